"""A numpy restatement of the cut's integer (int8-limb) MFMA pass: the quantisation of
sqlp_amd/csrc/cut_i8.h, the kept limb-pair dot product, the level combination and the band term.
Integer sums do not depend on their order, so the model gives the device's fp32 score term bit for
bit (tests/test_gpu_cut_i8.py) and the header's (tests/test_cut_i8_model.py, through
tests/native/cut_i8_check.cpp).  A plain helper module."""
import numpy as np

E_MIN = -64


def kq(L):
    return 7 * L - 1


def scale_exp(a):
    """The least exponent E >= E_MIN with a <= 2^E, elementwise (a >= 0 finite; 0 gives E_MIN)."""
    a = np.asarray(a, dtype=np.float64)
    f, e = np.frexp(a)
    e = np.where(f == 0.5, e - 1, e)
    return np.where(a > 0.0, np.maximum(e, E_MIN), E_MIN).astype(np.int64)


def quantise(a, E, L):
    """q = rint(a 2^(kQ - E)) (round half to even, as rint)."""
    return np.rint(np.ldexp(np.asarray(a, dtype=np.float64), kq(L) - np.asarray(E))).astype(np.int64)


def limbs(q, L):
    """The L balanced radix-128 digits of q, most significant first: shape q.shape + (L,)."""
    q = np.asarray(q, dtype=np.int64).copy()
    out = np.zeros(q.shape + (L,), dtype=np.int64)
    for j in range(L - 1):
        d = ((q + 64) & 127) - 64
        out[..., L - 1 - j] = d
        q = (q - d) >> 7
    out[..., 0] = q
    return out


def dropped_pairs(L):
    return sum(64.0 * 64.0 * 128.0 ** (2 * L - 2 - l1 - l2)
               for l1 in range(1, L) for l2 in range(1, L) if l1 + l2 >= L)


def band_term(k, S, nsum, L):
    """cut_i8.h band_term: the bound on |t - sum_e pc_e d_e| of a vertex with scale exponent S and
    normalised operand sum nsum."""
    R = sum((lv + 1) * 128.0 ** (2 * L - 2 - lv) for lv in range(L)) * k * 64.0 * 64.0
    u32 = 2.0 ** -24
    units = np.ldexp(np.asarray(nsum, dtype=np.float64), kq(L) - 1) + 0.25 * k + k * dropped_pairs(L) + (L - 1) * u32 * R * (1.0 + u32)
    return np.ldexp(units, np.asarray(S) - 2 * kq(L))


def operands(pc, dmax, L):
    """(E[k], S[nv], limbs of the vertex side [nv, k, L]) of pc[nv, k] = fl(PK coef) and dmax[k]."""
    pc = np.asarray(pc, dtype=np.float64)
    E = scale_exp(dmax)
    u = np.abs(np.ldexp(pc, E[None, :]))
    S = scale_exp(u.max(axis=1) if pc.shape[1] else np.zeros(len(pc)))
    qa = quantise(pc, S[:, None] - E[None, :], L)
    return E, S, limbs(qa, L)


def vertex_band(pc, dmax, L):
    """band_term of every vertex, with nsum as cut_vbase_kernel forms it."""
    pc = np.asarray(pc, dtype=np.float64)
    dmax = np.asarray(dmax, dtype=np.float64)
    E = scale_exp(dmax)
    S = scale_exp(np.abs(np.ldexp(pc, E[None, :])).max(axis=1))
    # summed in element order, as the header's check program does (cumsum adds sequentially)
    nsum = np.cumsum(np.ldexp(dmax, -E)[None, :] + np.ldexp(np.abs(pc), E[None, :] - S[:, None]), axis=1)[:, -1]
    return band_term(pc.shape[1], S, nsum, L)


def scores(pc, dv, dmax, L):
    """The pass's fp32 score terms t[N, nv] of deltas dv[N, k] (|dv[:, e]| <= dmax[e])."""
    pc = np.asarray(pc, dtype=np.float64)
    dv = np.asarray(dv, dtype=np.float64)
    E, S, la = operands(pc, dmax, L)
    ld = limbs(quantise(dv, E[None, :], L), L)                       # [N, k, L]
    f = None
    for lv in range(L):
        acc = np.zeros((dv.shape[0], pc.shape[0]), dtype=np.int64)
        for l1 in range(lv + 1):
            acc += ld[:, :, lv - l1] @ la[:, :, l1].T
        assert np.abs(acc).max(initial=0) < 2 ** 24            # exact in fp32
        # fmaf(f, 128, acc): f 128 + acc is exact in fp64 (integers below 2^53), one rounding to fp32
        f = acc.astype(np.float32) if f is None else (f.astype(np.float64) * 128.0 + acc).astype(np.float32)
    return f * np.ldexp(np.float32(1.0), S + 7 * (L - 1) - 2 * kq(L)).astype(np.float32)[None, :]
