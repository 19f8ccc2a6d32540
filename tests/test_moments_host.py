"""twosd_moments_merge (host code of the library, no GPU): the one merge behind the kernel's block
records, the chunks, the batches and the ranks of the out-of-sample estimator, against moments
taken in np.longdouble; and the argument checks of twosd_evaluate_ci that need no device."""
import ctypes as C

import numpy as np
import pytest

from sqlp_amd import _lib, twosd


def _moments(v):
    """Moments of v in long double, rounded to fp64 at the end."""
    v = np.asarray(v, dtype=np.longdouble)
    if v.size == 0:
        return twosd.Moments()
    mean = v.sum() / v.size
    return twosd.Moments(int(v.size), 0, float(mean), float(((v - mean) ** 2).sum()), float(v.min()), float(v.max()))


def _c_merge(a, b, alias=False):
    lib = _lib.load()
    ca, cb = a._c(), b._c()
    out = ca if alias else _lib.Moments()
    assert lib.twosd_moments_merge(C.byref(ca), C.byref(cb), C.byref(out)) == 0
    return twosd.Moments._of(out)


def _close(got, ref, m2_input_err=0.0, tol=1e-12):
    assert got.n == ref.n and got.n_bad == ref.n_bad
    assert abs(got.mean - ref.mean) <= tol * (1 + abs(ref.mean))
    assert abs(got.m2 - ref.m2) <= tol * (1 + abs(ref.m2)) + m2_input_err
    assert got.min == ref.min and got.max == ref.max


@pytest.mark.parametrize("na,nb", [(1, 1), (1, 1000), (1000, 1), (317, 4096), (5, 7)])
@pytest.mark.parametrize("loc", [0.0, 250.0, 1e6])
def test_merge_matches_longdouble_of_concatenation(na, nb, loc):
    """Tolerance: 1e-12 relative for the merge's own roundings (a handful of 2^-53), plus what the
    operands bring: each input mean is the long-double mean rounded to fp64, off by up to
    2^-53 |mean|, so d = mean_b - mean_a is off by e <= 2^-52 max|mean| and the update term
    d^2 na nb / n by 2 |d| e na nb / n (1e-10-sized at loc = 1e6: no defect of the merge)."""
    rng = np.random.default_rng(na * 7919 + nb)
    a = loc + rng.normal(size=na)
    b = loc + 0.5 + 2.0 * rng.normal(size=nb)
    ma, mb = _moments(a), _moments(b)
    e = 2.0 ** -52 * max(abs(ma.mean), abs(mb.mean))
    got = _c_merge(ma, mb)
    _close(got, _moments(np.concatenate([a, b])), m2_input_err=2 * abs(mb.mean - ma.mean) * e * na * nb / (na + nb))


def test_identity_operands_bit_for_bit():
    m = twosd.Moments(41, 3, 0.1 + 0.2, 1.0 / 3.0, -7.25, 1e300)
    empty = twosd.Moments(0, 5)
    for got in (_c_merge(m, empty), _c_merge(empty, m)):
        assert got == twosd.Moments(41, 8, m.mean, m.m2, m.min, m.max)
    both = _c_merge(empty, twosd.Moments(0, 2))
    assert both == twosd.Moments(0, 7, 0.0, 0.0, np.inf, -np.inf)
    # equal means: the update term vanishes exactly
    k = twosd.Moments(3, 0, 174.65, 0.0, 174.65, 174.65)
    assert _c_merge(k, k) == twosd.Moments(6, 0, 174.65, 0.0, 174.65, 174.65)


def test_out_may_alias_a():
    rng = np.random.default_rng(2)
    a, b = _moments(rng.normal(size=33)), _moments(3.0 + rng.normal(size=12))
    assert _c_merge(a, b, alias=True) == _c_merge(a, b)


def test_three_way_chain_equals_python_merge():
    rng = np.random.default_rng(3)
    parts = [_moments(100.0 + rng.normal(size=n)) for n in (257, 1, 4000)]
    parts[1] = twosd.Moments(parts[1].n, 4, parts[1].mean, parts[1].m2, parts[1].min, parts[1].max)
    c = _c_merge(_c_merge(parts[0], parts[1]), parts[2])
    py = parts[0].merge(parts[1]).merge(parts[2])
    assert c == py and py.n == 4258 and py.n_bad == 4
    # the derived quantities
    assert py.variance == py.m2 / (py.n - 1)
    assert py.std_error == pytest.approx(np.sqrt(py.variance / py.n), rel=1e-15)
    assert py.half_width(1.96) == pytest.approx(1.96 * py.std_error, rel=1e-15)
    assert np.isnan(twosd.Moments(1, 0, 2.0, 0.0, 2.0, 2.0).variance)


def test_merge_rejects_null():
    lib = _lib.load()
    m = _lib.Moments()
    assert lib.twosd_moments_merge(None, C.byref(m), C.byref(m)) == -1
    assert lib.twosd_moments_merge(C.byref(m), C.byref(m), None) == -1


def test_evaluate_ci_argument_checks_without_gpu():
    lib = _lib.load()
    m, hw, cv = _lib.Moments(), C.c_double(), C.c_int()

    def call(ctx=None, batch=1024, n_max=4096, z=1.96, rel=1e-3, ab=0.0, out=m):
        return lib.twosd_evaluate_ci(ctx, None, C.c_uint64(1), 0, batch, n_max, z, rel, ab, 0.0,
                                     None if out is None else C.byref(out), C.byref(hw), C.byref(cv))

    assert call(batch=1) == -1                # TWOSD_E_ARG
    assert call(batch=4096, n_max=4095) == -1
    assert call(z=0.0) == -1 and call(z=-1.0) == -1 and call(z=float("nan")) == -1
    assert call(rel=-1e-3) == -1 and call(ab=-1.0) == -1
    assert call(out=None) == -1
    assert b"batch" in lib.twosd_last_error() or b"evaluate_ci" in lib.twosd_last_error()
    assert call() == -3                       # good arguments, no context: TWOSD_E_STATE
    for f, args in ((lib.twosd_evaluate_moments, (None, None, 0, 16, C.c_uint64(1), C.byref(m))),
                    (lib.twosd_evaluate_paired, (None, None, None, 0, 16, C.c_uint64(1), C.byref(m), C.byref(m), C.byref(m))),
                    (lib.twosd_moments_of_values, (None, 0, None, None, C.byref(m)))):
        assert f(*args) in (-1, -3)
    with pytest.raises(ValueError):
        twosd.normal_quantile(1.0)
    assert twosd.normal_quantile(0.95) == pytest.approx(1.959963984540054, rel=1e-12)
