"""Host restatement (numpy) of the variance-reduced scenario streams and of the grouped moments
(DESIGN.md §5.9): the reference of tests/test_gpu_vr_*.py.  Shares no code with the library:
Philox4x32-10 is restated from Salmon et al. (SC'11) and pinned against the oracle's C restatement
in tests/test_vr_host.py; the inverse normal CDF is Newton's iteration on math.erfc.

A distribution table `dists` is a list over the random elements (position order) of
("DISCRETE", values, probs) / ("NORMAL", mean, variance) / ("UNIFORM", left, right), the entries of
spStoType.indep.  All functions return element VALUES (not deltas), shape (N, k)."""
import math
from statistics import NormalDist

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
ONE_MINUS = 1.0 - 2.0 ** -53      # the largest double below 1
U_FLOOR = 2.0 ** -54              # the NORMAL inversion's lower clamp


def philox4x32_10(c0, c1, c2, c3, seed):
    """Philox4x32-10 of the counters (arrays broadcast together) under key (seed_lo, seed_hi):
    four uint64 arrays holding the 32-bit output words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3)])
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def _u01(a, b):
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53


def uniforms(seed, g, k):
    """(u1, u2), each (len(g), k): the sampler's uniforms of global indices g, elements 0..k-1."""
    g = np.asarray(g, dtype=np.uint64)[:, None]
    e = np.arange(k, dtype=np.uint64)[None, :]
    w = philox4x32_10(g & _M32, g >> np.uint64(32), e, 0, seed)
    return _u01(w[0], w[1]), _u01(w[2], w[3])


def _sorted_support(d):
    order = np.argsort(np.asarray(d[1], dtype=np.float64), kind="stable")
    return np.asarray(d[1], dtype=np.float64)[order], np.asarray(d[2], dtype=np.float64)[order]


def invert(d, u):
    """A DISCRETE or UNIFORM element at the uniforms u (the i.i.d. sampler's arithmetic)."""
    u = np.asarray(u, dtype=np.float64)
    if d[0] == "DISCRETE":
        val, prob = _sorted_support(d)
        cp = np.full(u.shape, prob[0])
        i = np.zeros(u.shape, dtype=np.int64)
        go = np.ones(u.shape, dtype=bool)
        for j in range(1, len(val)):
            go &= cp <= u                      # the walk stops for good at the first cp > u
            cp = np.where(go, cp + prob[j], cp)
            i += go
        return val[i]
    assert d[0] == "UNIFORM"
    left, right = float(d[1]), float(d[2])
    return left + (right - left) * u


def box_muller(u1, u2):
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(6.283185307179586 * u2)


def ncdfinv(u):
    """Phi^-1(u), 0 < u < 1: Newton on Phi(z) = erfc(-z / sqrt 2) / 2 to convergence, on the lower
    tail (u > 1/2 by symmetry, 1 - u being exact there), where erfc keeps its relative accuracy."""
    if u > 0.5:
        return -ncdfinv(1.0 - u)
    z = NormalDist().inv_cdf(u) if u > 1e-300 else -37.0
    for _ in range(60):
        f = 0.5 * math.erfc(-z / math.sqrt(2.0)) - u
        dz = f / (math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi))
        z -= dz
        if abs(dz) <= 1e-17 * max(1.0, abs(z)):
            break
    return z


def iid(dists, N, seed, first=0):
    k = len(dists)
    u1, u2 = uniforms(seed, first + np.arange(N, dtype=np.uint64), k)
    out = np.empty((N, k))
    for e, d in enumerate(dists):
        if d[0] == "NORMAL":
            out[:, e] = d[1] + math.sqrt(d[2]) * box_muller(u1[:, e], u2[:, e])
        else:
            out[:, e] = invert(d, u1[:, e])
    return out


def antithetic(dists, N, seed, first=0):
    """Pair p = g >> 1 uses the words of index 2p; the odd member mirrors the even one."""
    assert first % 2 == 0 and N % 2 == 0
    k = len(dists)
    g = np.uint64(first) + np.arange(N, dtype=np.uint64)
    odd = (g & np.uint64(1)).astype(bool)
    u1, u2 = uniforms(seed, g & ~np.uint64(1), k)
    out = np.empty((N, k))
    for e, d in enumerate(dists):
        if d[0] == "NORMAL":
            z = box_muller(u1[:, e], u2[:, e])
            out[:, e] = d[1] + math.sqrt(d[2]) * np.where(odd, -z, z)
        else:
            out[:, e] = invert(d, np.where(odd, 1.0 - u1[:, e], u1[:, e]))
    return out


def lhs_permutations(S, blocks, k, seed):
    """perm[b, e, :]: the permutation of 0..S-1 of global block blocks[b], element e (inside-out
    Fisher-Yates from Philox counters (b_lo, b_hi, e, 2 + (i >> 2)), word i & 3)."""
    b = np.asarray(blocks, dtype=np.uint64)[:, None]
    e = np.arange(k, dtype=np.uint64)[None, :]
    perm = np.zeros((b.shape[0], k, S), dtype=np.int64)
    words = None
    for i in range(1, S):
        if i == 1 or i % 4 == 0:
            words = philox4x32_10(b & _M32, b >> np.uint64(32), e, 2 + (i >> 2), seed)
        t = ((words[i & 3] * np.uint64(i + 1)) >> np.uint64(32)).astype(np.int64)[..., None]
        np.put_along_axis(perm, np.full_like(t, i), np.take_along_axis(perm, t, axis=2), axis=2)
        np.put_along_axis(perm, t, i, axis=2)
    return perm


def lhs_uniforms(S, N, k, seed, first=0):
    """u (N, k) of the LHS stream: min((perm[j] + u1(g, e)) / S, 1 - 2^-53)."""
    assert first % S == 0 and N % S == 0
    nb = N // S
    perm = lhs_permutations(S, first // S + np.arange(nb), k, seed)       # (nb, k, S)
    u1, _ = uniforms(seed, first + np.arange(N, dtype=np.uint64), k)
    strata = perm.transpose(0, 2, 1).reshape(N, k).astype(np.float64)    # row b S + j = perm[b, :, j]
    return np.minimum((strata + u1) / float(S), ONE_MINUS)


def lhs(dists, S, N, seed, first=0):
    k = len(dists)
    u = lhs_uniforms(S, N, k, seed, first)
    out = np.empty((N, k))
    for e, d in enumerate(dists):
        if d[0] == "NORMAL":
            z = np.array([ncdfinv(max(float(v), U_FLOOR)) for v in u[:, e]])
            out[:, e] = d[1] + math.sqrt(d[2]) * z
        else:
            out[:, e] = invert(d, u[:, e])
    return out


def dists_of(sto, positions):
    return [sto.indep[p] for p in positions]


# ---- grouped moments ---------------------------------------------------------------------------
def group_means(v, G):
    """The library's group mean, bit for bit: K = v[0]; s = 0.0; s += v[i] - K for i = 0..G-1 in
    order; mean = K + s / G (every operation one fp64 rounding)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, G)
    K = v[:, 0].copy()
    s = np.zeros(v.shape[0])
    for i in range(G):
        s = s + (v[:, i] - K)
    return K + s / float(G)


def grouped(v, status, G):
    """(means of the counted groups, n_bad): a group counts when all G statuses are 0; the values
    of the others are not touched."""
    v = np.asarray(v, dtype=np.float64)
    ok = np.ones(v.size // G, dtype=bool) if status is None else (np.asarray(status).reshape(-1, G) == 0).all(axis=1)
    rows = v.reshape(-1, G)[ok]
    return (group_means(rows, G) if rows.size else np.zeros(0)), int((~ok).sum())
