"""Directed inputs of the quantile selection's tests (tests/test_risk_host.py on the restatement,
tests/test_gpu_risk_quantile.py on the device).  A plain helper module.

directed(n) -> {name: (values, weights or None, status or None)} of n entries each:
  equal       all values equal
  exact_hit   distinct values; weights 1 except one on the largest value that makes the total a power
              of two, so the integer weights are exact multiples of one unit and at level 0.5 the
              cumulative weight meets t = Q / 2 exactly at a value (n >= 3; unit weights otherwise)
  zeros       -0.0 and +0.0 only, alternating
  negative    negative values, denormals of both signs and a few normal values
  low_byte    bit patterns that differ in the lowest key byte only
  high_byte   bit patterns that differ in the highest key byte only
  weights     random values under non-uniform weights, about a quarter of them zero
  bad_nan     random values; about a fifth of the entries non-optimal with value NaN
"""
from __future__ import annotations

import numpy as np

SIZES = (1, 2, 255, 256, 257, 4097)
LEVELS = (0.5, 0.9, 1.0 - 2.0 ** -20)


def _from_bits(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def directed(n: int) -> dict:
    rng = np.random.default_rng(1000 + n)
    out = {}
    out["equal"] = (np.full(n, 3.25), None, None)
    vals = rng.permutation(n).astype(np.float64) - n / 3.0
    w = np.ones(n)
    if n >= 3:
        total = 1 << int(np.floor(np.log2(2 * n - 2)))      # n <= total <= 2 n - 2: half of it lies among the unit weights
        w[int(np.argmax(vals))] = total - (n - 1)
    out["exact_hit"] = (vals, w, None)
    z = np.zeros(n)
    z[::2] = -0.0
    out["zeros"] = (z, None, None)
    neg = -np.abs(rng.normal(size=n)) * 10.0 ** rng.integers(-3, 4, size=n)
    den = rng.integers(1, 50, size=n) * 5e-324 * rng.choice([-1.0, 1.0], size=n)
    out["negative"] = (np.where(rng.uniform(size=n) < 0.5, neg, den), None, None)
    base = np.uint64(0x4059123456789A00)
    out["low_byte"] = (_from_bits(base + (rng.permutation(n) % 200).astype(np.uint64)), None, None)
    hi = (rng.permutation(n) % 256).astype(np.uint64)
    out["high_byte"] = (_from_bits((hi << np.uint64(56)) | np.uint64(0x0051234567890ABC)), None, None)
    ww = rng.uniform(0.1, 3.0, size=n) * (rng.uniform(size=n) >= 0.25)
    if not ww.any():
        ww[0] = 1.0
    out["weights"] = (rng.normal(size=n) * 100.0, ww, None)
    st = (rng.uniform(size=n) < 0.2).astype(np.int32) * rng.integers(1, 4, size=n).astype(np.int32)
    if st.all():
        st[0] = 0
    v = rng.normal(size=n)
    v[st != 0] = np.nan
    out["bad_nan"] = (v, rng.uniform(0.5, 1.5, size=n), st)
    return out
