"""Python restatement of the risk kernels (sqlp_amd/csrc/risk.hip), shared by tests/test_risk_host.py
and the tests/test_gpu_risk_*.py files.  A plain helper module.

* quantile: Python integers and fractions.Fraction throughout -- the integer weights
  q_s = rn(w_s * rn(2^58 / W)) (W the weights' fp64 sum in index order; 1 without weights), the
  exact threshold t = ceil(level * Q), VaR by a walk over the entries sorted by their
  sign-flipped bit patterns (so -0 sorts before +0), tail_q, and CVaR as an exact rational
  rounded once.
* tail_cut: boot_ref.reform with the counts c = (max_val > eta), returning W_t as well.
"""
from __future__ import annotations

import math
import struct
from fractions import Fraction

import numpy as np

from tests import boot_ref

FIX = 2.0 ** 58


def key(v: float) -> int:
    """The order-preserving 64-bit key of an fp64 value (risk_keys.h: risk_key)."""
    b = struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def unkey(k: int) -> float:
    b = k & 0x7FFFFFFFFFFFFFFF if k >> 63 else (~k) & 0xFFFFFFFFFFFFFFFF
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def total_weight(weights) -> float:
    """The weights' sum in index order, every add rounded (an epigraph's running total)."""
    t = 0.0
    for w in np.asarray(weights, dtype=np.float64):
        t = t + float(w)
    return t


def int_weights(weights, total=None):
    """q_s = rn(w_s * rn(2^58 / total)) as Python ints (w <= 0 weighs nothing)."""
    w = np.asarray(weights, dtype=np.float64)
    total = total_weight(w) if total is None else float(total)
    scale = FIX / total
    return [int(np.rint(x * scale)) if x > 0.0 else 0 for x in w]


def threshold(level: float, Q: int) -> int:
    """ceil(level * Q), exact."""
    return math.ceil(Fraction(float(level)) * Q)


def quantile(values, weights, status, level, total=None):
    """(var, cvar, tail_q, total_q, n_bad) as twosd_quantile_of_values defines them; None when no
    entry counts.  total: the weights' scale total (default: their sum in index order)."""
    values = np.asarray(values, dtype=np.float64).ravel()
    n = len(values)
    q = [1] * n if weights is None else int_weights(weights, total)
    ok = [True] * n if status is None else [int(s) == 0 for s in np.asarray(status).ravel()]
    n_bad = n - sum(ok)
    ent = sorted((key(values[s]), q[s]) for s in range(n) if ok[s])
    Q = sum(e[1] for e in ent)
    if not ent or Q == 0:
        return None
    t = threshold(level, Q)
    cum, vkey = 0, None
    for kk, qq in ent:
        cum += qq
        if cum >= t:
            vkey = kk
            break
    var = unkey(vkey)
    tail = [(unkey(kk), qq) for kk, qq in ent if kk > vkey]
    tail_q = sum(qq for _, qq in tail)
    num = sum((Fraction(v) - Fraction(var)) * qq for v, qq in tail)
    cvar = float(Fraction(var) + num / ((1 - Fraction(float(level))) * Q))
    return var, cvar, tail_q, Q, n_bad


def brute_quantile(values, q, level):
    """The definition by a plain numeric sort (no keys): the smallest value whose cumulative
    integer weight reaches ceil(level Q).  Ties between -0 and +0 are not ordered here."""
    order = np.argsort(np.asarray(values, dtype=np.float64), kind="stable")
    Q = sum(q)
    t = threshold(level, Q)
    cum = 0
    for s in order:
        cum += q[s]
        if cum >= t:
            return float(values[s])
    raise AssertionError("unreachable")


def tail_cut(r, T, c0, rows, cols, V, dv, w, picks, max_val, eta):
    """(alpha, beta, W_t) of the tail cut: boot_ref.reform with the counts 1[max_val > eta]."""
    c = (np.asarray(max_val, dtype=np.float64) > float(eta)).astype(np.float64)
    return boot_ref.reform(r, T, c0, rows, cols, V, dv, w, picks, c=c)
