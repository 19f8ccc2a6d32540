"""The device quantile selection (sqlp_amd/csrc/risk.hip: twosd_quantile_of_values) against the
integer / Fraction restatement tests/risk_ref.quantile on the directed inputs of tests/risk_cases.py.

VaR, tail_q, total_q and n_bad are compared bit for bit; cvar to the project's cut tolerance
1e-8 (1 + |ref|) (the device sums fp64 products in a fixed shard order, the restatement is an exact
rational rounded once).  Every result must be identical under two other launch grids
(TWOSD_RISK_BLOCKS).  Sizes: around one block and around the 256-bin histogram."""
import contextlib
import os
import struct

import numpy as np
import pytest

from tests import instances as I
from tests import risk_cases as RC
from tests import risk_ref as RR

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


@pytest.fixture(scope="module")
def ctx():
    from sqlp_amd import twosd
    inst = I.load("lands")
    c = twosd.SDContext(inst["sp2"], inst["sto"])
    yield c
    c.close()


@pytest.mark.parametrize("n", RC.SIZES)
def test_quantile_matches_the_restatement_bit_for_bit(ctx, n):
    from sqlp_amd import twosd
    worst = 0.0
    for name, (vals, w, st) in RC.directed(n).items():
        for level in RC.LEVELS:
            var, cvar, tail_q, Q, n_bad = RR.quantile(vals, w, st, level)
            got = twosd.quantile_of_values(ctx, vals, level, weights=w, status=st)
            what = (name, n, level)
            assert _bits(got.var) == _bits(var), what                      # the bits: -0 and +0 differ
            assert (got.tail_q, got.total_q, got.n_bad) == (tail_q, Q, n_bad), what
            err = abs(got.cvar - cvar) / (1e-8 * (1 + abs(cvar)))
            worst = max(worst, err)
            assert err <= 1.0, (what, got.cvar, cvar)
            for blocks in ("1", "3"):
                with _env(TWOSD_RISK_BLOCKS=blocks):
                    g2 = twosd.quantile_of_values(ctx, vals, level, weights=w, status=st)
                assert (_bits(g2.var), _bits(g2.cvar), g2.tail_q, g2.total_q, g2.n_bad) == \
                       (_bits(got.var), _bits(got.cvar), got.tail_q, got.total_q, got.n_bad), (what, blocks)
    print(f"n = {n}: worst cvar error {worst:.3e} of the bound")


def test_each_radix_pass_decides_once(ctx):
    """Two values whose keys differ in byte p only, p = 0 (lowest) .. 7: the selection must tell them
    apart in exactly that pass.  Unit weights, level 0.5 picks the lower one, 0.9 the upper."""
    from sqlp_amd import twosd
    base = 0x4051234567890ABC
    for p in range(8):
        other = base ^ (0x01 << (8 * p)) if p < 7 else base ^ (0x40 << 56)    # stays a finite positive double
        lo, hi = sorted([base, other])
        vals = np.array([hi, lo], dtype=np.uint64).view(np.float64)
        for level, want in ((0.5, lo), (0.9, hi)):
            got = twosd.quantile_of_values(ctx, vals, level)
            assert _bits(got.var) == want, (p, level)
            assert got.tail_q == (1 if want == lo else 0) and got.total_q == 2


def test_argument_errors(ctx):
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    v = np.array([1.0, 2.0, 3.0])
    for level in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(TwoSDError) as e:
            twosd.quantile_of_values(ctx, v, level)
        assert e.value.code == -1
    with pytest.raises(TwoSDError) as e:
        twosd.quantile_of_values(ctx, np.zeros(0), 0.5)
    assert e.value.code == -1
    with pytest.raises(TwoSDError) as e:                                       # no entry counts
        twosd.quantile_of_values(ctx, v, 0.5, status=np.array([1, 2, 3]))
    assert e.value.code == -1
    with pytest.raises(TwoSDError) as e:
        twosd.quantile_of_values(ctx, v, 0.5, weights=np.zeros(3))
    assert e.value.code == -1
    with pytest.raises(TwoSDError) as e:
        twosd.quantile_of_values(ctx, v, 0.5, weights=np.array([1.0, -1.0, 1.0]))
    assert e.value.code == -1
    with pytest.raises(ValueError):
        twosd.quantile_of_values(ctx, v, 0.5, weights=np.ones(2))
    # the one counted entry is the quantile at every level
    got = twosd.quantile_of_values(ctx, np.array([np.nan, 7.5, np.nan]), 0.9, status=np.array([3, 0, 1]))
    assert (got.var, got.cvar, got.tail_q, got.total_q, got.n_bad) == (7.5, 7.5, 0, 1, 2)
