"""numpy restatement of the bootstrap re-formation (sqlp_amd/csrc/boot_kernel.hip), shared by
tests/test_boot_host.py and tests/test_gpu_bootstrap.py.  A plain helper module.

* counts: Philox4x32-10 from the oracle's C restatement (oracle.cpu.philox4x32_10), counter
  (g_lo, g_hi, b >> 2, 1), key (seed_lo, seed_hi), word b & 3, through the 12 thresholds of the
  Poisson(1) CDF.
* the cut from picks: the weights W and the per-vertex weights by math.fsum (exact), the element
  sums S_e and g in numpy's extended precision (np.longdouble: products of fp64 values summed with
  a 64-bit significand, an error below 1e-15 of the sums' magnitude at these sizes), then
  build_sasa_cut's formula (epigraph.jl:125-146) with the picks fixed.
"""
from __future__ import annotations

import functools
import math

import numpy as np

THRESHOLDS = [0x5e2d58d9, 0xbc5ab1b1, 0xeb715e1e, 0xfb239797, 0xff1025f6, 0xffd90f3c,
              0xfffa8b72, 0xffff540c, 0xffffed1f, 0xfffffe21, 0xffffffd5, 0xfffffffc]


def count_of_word(u: int) -> int:
    return sum(1 for t in THRESHOLDS if u >= t)


@functools.lru_cache(maxsize=None)
def counts(seed: int, first: int, count: int, M: int) -> np.ndarray:
    """uint8 (count, M): replicate b's count of the scenario with global index first + s."""
    from oracle import cpu
    thr = np.array(THRESHOLDS, dtype=np.uint64)
    out = np.zeros((count, M), dtype=np.uint8)
    key = [seed & 0xffffffff, (seed >> 32) & 0xffffffff]
    for s in range(count):
        g = (first + s) & 0xffffffffffffffff
        for Q in range((M + 3) // 4):
            w = cpu.philox4x32_10([g & 0xffffffff, g >> 32, Q, 1], key)
            for t in range(4):
                if 4 * Q + t < M:
                    out[s, 4 * Q + t] = int((np.uint64(w[t]) >= thr).sum())
    out.setflags(write=False)
    return out


def reform(r, T, c0, rows, cols, V, dv, w, picks, c=None):
    """(alpha, beta, W) of the cut over the first len(picks) scenarios with counts c (None: all 1).
    r (mv), T (mv x n1): the LP's (canonical) rhs and technology matrix; rows / cols (k): the
    random elements' rows and first-stage columns (-1: rhs); V (|V| x mv); dv (N x k) deltas;
    w (N) weights."""
    n = len(picks)
    n1 = T.shape[1]
    c = np.ones(n) if c is None else np.asarray(c, dtype=np.float64)
    cw = c * np.asarray(w[:n], dtype=np.float64)          # exact: small integers times fp64
    W = math.fsum(cw)
    if W == 0.0:
        return 0.0, np.zeros(n1), 0.0
    LD = np.longdouble
    hv = {}
    for s in range(n):
        hv.setdefault(int(picks[s]), []).append(cw[s])
    g = np.zeros(V.shape[1], dtype=LD)
    for v, ws in hv.items():
        g += LD(math.fsum(ws)) * V[v].astype(LD)
    k = len(rows)
    S = np.zeros(k, dtype=LD)
    if k:
        PK = V[np.asarray(picks, dtype=np.int64)][:, rows].astype(LD)       # n x k
        S = (cw.astype(LD)[:, None] * PK * dv[:n].astype(LD)).sum(axis=0)
    a = (g * r.astype(LD)).sum()
    beta = -(T.astype(LD).T @ g)
    for e in range(k):
        if cols[e] < 0:
            a += S[e]
        else:
            beta[cols[e]] -= S[e]
    return float(a / LD(W)) + c0, (beta / LD(W)).astype(np.float64), W


def epigraph_value(cuts, incumbent, x, total_weight, lower_bound):
    """evaluate_epigraph (epigraph.jl:177-203, MIN sense) over (alpha, beta, weight_mark) triples."""
    best = lower_bound
    for a, b, wm in cuts:
        d = wm / total_weight
        best = max(best, d * (a + float(np.dot(b, x))) + (1 - d) * lower_bound)
    if incumbent is not None:
        best = max(best, incumbent[0] + float(np.dot(incumbent[1], x)))
    return best
