"""Out-of-sample CVaR on the device (twosd_evaluate_cvar) on data/smps/lands3b at lands' x_EV,
n = 65 536 scenarios of one seed, level 0.8:

* var is, bit for bit, the ceil(level n)-th smallest of the objectives solve_values returns for the
  same stream (add_sampled_scenarios + get_scenarios);
* y is, bit for bit, moments_of_values of the numpy-formed Y = var + max(obj - var, 0) / (1 - level)
  (one chunk: one reduction over the whole range);
* |cvar - exact| <= 4 std_error against the CVaR enumerated over the six realisations with HiGHS --
  four standard errors of the estimator itself, not a tuned bound;
* a second call returns the same bits."""
import math
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

from tests import instances as I

pytestmark = pytest.mark.gpu

N, SEED, LEVEL = 65536, 4242, 0.8


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


@pytest.fixture(scope="module")
def L():
    from types import SimpleNamespace
    from sqlp_amd import smps, twosd
    cor, tim, sto = smps.load_smps(os.path.join(I.DATA, "lands3b"))
    sp2 = smps.get_smps_stage_template(cor, tim, 2)
    ctx = twosd.SDContext(sp2, sto)
    ctx.set_distributions(sto)
    x = I.x_ev("lands")
    ctx.compute_basis(x, smps.mean_values(sto))
    c1 = np.asarray(smps.get_smps_stage_template(cor, tim, 1).q, dtype=np.float64)
    support, probs = smps.joint_support(sto, ctx.positions)
    yield SimpleNamespace(ctx=ctx, x=x, c1=c1, support=support, probs=np.asarray(probs) / np.sum(probs))
    ctx.close()


def _exact_cvar(L, level):
    """min over eta of eta + E[(h - eta)+] / (1 - level) over the support (attained at an atom), h by HiGHS."""
    from oracle import lp_highs
    sp = I.load("lands")["osp2"]
    h = []
    for v in L.support:
        b = sp.r - sp.T @ L.x
        b[L.ctx.rows] += v - sp.r[L.ctx.rows]
        st, o, _, _ = lp_highs.solve_rhs(sp, b)
        assert st == 0
        h.append(o)
    h = np.array(h)
    return min(float(eta + L.probs @ np.maximum(h - eta, 0.0) / (1.0 - level)) for eta in h)


def test_evaluate_cvar_on_lands3b(L):
    from sqlp_amd import twosd
    ctx, x = L.ctx, L.x
    zero = np.zeros(len(x))
    res = twosd.evaluate_cvar(ctx, zero, x, SEED, 0, N, LEVEL)
    assert res.n == N and res.n_bad == 0
    # the same stream through an epigraph and solve_values
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, N, SEED, first_index=0)
    obj, _, _, st = ctx.solve_values(x, twosd.get_scenarios(epi), want_pi=False)
    assert (st == 0).all()
    kth = math.ceil(Fraction(LEVEL) * N)
    assert _bits(res.var) == _bits(np.sort(obj)[kth - 1])
    Y = res.var + np.maximum(obj - res.var, 0.0) / (1.0 - LEVEL)
    m = twosd.moments_of_values(ctx, Y)
    for f in ("n", "n_bad"):
        assert getattr(res.y, f) == getattr(m, f)
    for f in ("mean", "m2", "min", "max"):
        assert _bits(getattr(res.y, f)) == _bits(getattr(m, f)), f
    assert _bits(res.cvar) == _bits(m.mean) and res.std_error == m.std_error
    assert res.half_width(2.0) == 2.0 * res.std_error
    # against the enumerated CVaR
    exact = _exact_cvar(L, LEVEL)
    z = (res.cvar - exact) / res.std_error
    print(f"evaluate_cvar lands3b: var {res.var:.6f}, cvar {res.cvar:.6f}, exact {exact:.6f}, standard error {res.std_error:.5f}, z = {z:.2f}")
    assert abs(res.cvar - exact) <= 4.0 * res.std_error
    # the first-stage cost shifts var, cvar and the moments
    shifted = twosd.evaluate_cvar(ctx, L.c1, x, SEED, 0, N, LEVEL)
    c = float(L.c1 @ x)
    assert shifted.var == res.var + c and shifted.cvar == res.cvar + c and _bits(shifted.y.m2) == _bits(res.y.m2)
    # the same bits again
    again = twosd.evaluate_cvar(ctx, zero, x, SEED, 0, N, LEVEL)
    assert again == res


def test_evaluate_cvar_refusals(L):
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    ctx, x = L.ctx, L.x
    with pytest.raises(ValueError, match="i.i.d."):
        twosd.evaluate_cvar(ctx, L.c1, x, SEED, 0, 64, LEVEL, sampling=twosd.Sampling.antithetic())
    with pytest.raises(ValueError):
        twosd.evaluate_cvar(ctx, L.c1, x, SEED, 0, 64, 1.0)
    with pytest.raises(TwoSDError) as e:
        twosd.evaluate_cvar(ctx, L.c1, x, SEED, 0, (1 << 27) + 1, LEVEL)
    assert e.value.code == -5
    with pytest.raises(TwoSDError) as e:
        twosd.evaluate_cvar(ctx, L.c1, x, SEED, 0, 0, LEVEL)
    assert e.value.code == -1
    small = twosd.evaluate_cvar(ctx, L.c1, x, SEED, 0, 64, LEVEL, sampling=twosd.Sampling.iid())
    assert small.n == 64 and small.var <= small.cvar
