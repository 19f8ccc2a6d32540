"""twosd_canonical_form (host code of libtwosd_hip.so, no GPU call): general stage-2 bounds
removed into a plain y' >= 0 LP with extra rows for the boxed variables.  The canonical LP plus
c0 must have the bounded LP's optimum (HiGHS on both), its solution mapped back must lie within
the bounds at the same cost, default bounds must leave the arrays untouched bit for bit, and
bounds that are no interval are refused."""
import numpy as np
import pytest

from oracle import lp_highs
from tests import bounds_cases as BC


def _dense(csc, m, n):
    cp, rv, nz = csc
    A = np.zeros((m, n))
    for j in range(n):
        A[rv[cp[j]:cp[j + 1]], j] = nz[cp[j]:cp[j + 1]]
    return A


def test_toy_every_kind_matches_bounded_lp():
    from sqlp_amd import twosd
    K = twosd.canonical_form(BC.dense_to_csc(BC.TOY_W), BC.TOY_Q, BC.TOY_R, BC.TOY_SENSE, BC.TOY_LB, BC.TOY_UB)
    # shape: one bound row (the boxed column), the fixed column gone, one y- column for the free one
    assert (K.m_lp, K.n_lp, K.n_bound_rows) == (4, 6, 1)
    assert K.sense == ["G", "L", "E", "L"] and K.box_col.tolist() == [5]
    assert K.col_src.tolist() == [0, 1, 2, 3, -1, 4] and K.col_src2.tolist() == [-1, -1, -1, 5, -1, -1]
    # the library's arrays equal the table restated in numpy
    R = BC.canon_np(BC.TOY_W, BC.TOY_Q, BC.TOY_R, BC.TOY_SENSE, BC.TOY_LB, BC.TOY_UB)
    Wc = _dense(K.W, K.m_lp, K.n_lp)
    np.testing.assert_array_equal(Wc, R.W)
    np.testing.assert_array_equal(K.q, R.q)
    # r - W s: the library subtracts column by column, numpy subtracts the product; at most
    # n2 + 1 roundings of terms bounded by |r| + |W||s| apart
    np.testing.assert_allclose(K.r, R.r, rtol=0, atol=8 * np.finfo(float).eps * (np.abs(BC.TOY_R) + np.abs(BC.TOY_W) @ np.abs(R.s)).max())
    assert K.c0 == pytest.approx(R.c0, rel=1e-15)
    bounded = BC.highs_problem(BC.TOY_W, BC.TOY_Q, BC.TOY_SENSE, BC.TOY_LB, BC.TOY_UB)
    plain = BC.highs_problem(Wc, K.q, K.sense, np.zeros(K.n_lp), np.full(K.n_lp, np.inf))
    shift = BC.TOY_W @ R.s
    for v in BC.toy_values(16):
        b = v - BC.TOY_T @ BC.TOY_X
        st0, obj0, y0, _ = lp_highs.solve_rhs(bounded, b)
        b_lp = np.concatenate([b - shift, K.r[3:]])
        st1, obj1, y1, pi1 = lp_highs.solve_rhs(plain, b_lp)
        assert st0 == 0 and st1 == 0
        assert obj1 + K.c0 == pytest.approx(obj0, rel=1e-9, abs=1e-9)
        y = K.map_back(y1)
        assert (y >= BC.TOY_LB - 1e-9).all() and (y <= BC.TOY_UB + 1e-9).all()
        assert y[4] == 1.5                                     # the fixed column is its bound exactly
        assert float(BC.TOY_Q @ y) == pytest.approx(obj0, rel=1e-9, abs=1e-9)
        # the caller's rows hold for the mapped-back point
        lhs = BC.TOY_W @ y
        assert lhs[0] >= b[0] - 1e-9 and lhs[1] <= b[1] + 1e-9 and lhs[2] == pytest.approx(b[2], abs=1e-9)
        # the dual identity of the header: obj = v . [b - W s ; hi - lo] + c0, boxed multiplier <= 0
        assert float(pi1 @ b_lp) + K.c0 == pytest.approx(obj0, rel=1e-9, abs=1e-9)
        assert pi1[3] <= 1e-12


def test_default_bounds_are_a_noop_bit_for_bit():
    from sqlp_amd import twosd
    rng = np.random.default_rng(2)
    W = rng.normal(size=(5, 9)) * (rng.random((5, 9)) < 0.6)
    W[0, :] = rng.normal(size=9)                               # no empty column
    csc = BC.dense_to_csc(W)
    q, r = rng.normal(size=9), rng.normal(size=5)
    sense = ["G", "L", "E", "E", "G"]
    for lb, ub in [(None, None), (np.zeros(9), np.full(9, np.inf)), (-np.zeros(9), None)]:
        K = twosd.canonical_form(csc, q, r, sense, lb, ub)
        assert (K.m_lp, K.n_lp, K.n_bound_rows) == (5, 9, 0) and K.c0 == 0.0
        for a, b in zip(K.W, csc):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        assert K.q.tobytes() == q.tobytes() and K.r.tobytes() == r.tobytes() and K.sense == sense
        assert K.col_src.tolist() == list(range(9)) and (K.col_src2 == -1).all()
        assert (K.col_sign == 1.0).all() and (K.col_off == 0.0).all() and len(K.box_col) == 0


@pytest.mark.parametrize("j,lo,hi", [(2, 1.0, 0.5), (0, np.nan, 1.0), (1, 0.0, np.nan), (3, np.inf, np.inf),
                                     (4, -np.inf, -np.inf), (5, 0.0, -1.0)])
def test_bad_bounds_are_refused(j, lo, hi):
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    lb, ub = BC.TOY_LB.copy(), BC.TOY_UB.copy()
    lb[j], ub[j] = lo, hi
    with pytest.raises(TwoSDError) as ei:
        twosd.canonical_form(BC.dense_to_csc(BC.TOY_W), BC.TOY_Q, BC.TOY_R, BC.TOY_SENSE, lb, ub)
    assert ei.value.code == -1 and f"y[{j}]" in str(ei.value)       # TWOSD_E_ARG, naming j
