"""Host side of the stopping rule (no GPU): the Poisson(1) threshold table, the library's
twosd_bootstrap_count_of_word, and bootstrap_gap_test's arithmetic on a hand-made cell with an
injected re-formation."""
from decimal import ROUND_HALF_EVEN, Decimal, getcontext
from types import SimpleNamespace

import numpy as np
import pytest

from tests import boot_ref as BR
from tests import instances as I


def test_thresholds_are_the_rounded_poisson_cdf():
    getcontext().prec = 60
    e1 = Decimal(-1).exp()
    cdf, fact = Decimal(0), Decimal(1)
    for j, t in enumerate(BR.THRESHOLDS):
        if j:
            fact *= j
        cdf += e1 / fact
        assert int((cdf * (1 << 32)).quantize(Decimal(1), rounding=ROUND_HALF_EVEN)) == t, j
    # over the 2^32 words: mean exactly 1, second moment 2 + 1.4e-9
    p = np.diff(np.array([0] + BR.THRESHOLDS + [1 << 32], dtype=np.float64)) / 2.0 ** 32
    n = np.arange(13)
    assert sum((1 << 32) - t for t in BR.THRESHOLDS) == 1 << 32
    assert abs(float(p @ (n * n)) - 2.0) < 2e-9


def test_count_of_word_at_every_threshold():
    from sqlp_amd import twosd
    assert twosd.bootstrap_count_of_word(0) == 0
    assert twosd.bootstrap_count_of_word(2 ** 32 - 1) == 12
    for j, t in enumerate(BR.THRESHOLDS):
        assert twosd.bootstrap_count_of_word(t) == j + 1 == BR.count_of_word(t)
        assert twosd.bootstrap_count_of_word(t - 1) == j == BR.count_of_word(t - 1)


def _hand_cell():
    """lands' root stage with one epigraph holding a cut (weight 8 of 10) and an incumbent cut."""
    from sqlp_amd import master, smps, twosd
    inst = I.load("lands")
    sp1 = smps.get_smps_stage_template(inst["cor"], inst["tim"], 1)
    sp2 = inst["sp2"]
    row = sp2.stage_constraints.index("S2C5")
    rhs = []
    for v in (3.0, 5.0, 7.0):
        r = sp2.r.copy(); r[row] = v; rhs.append(r)
    _, x0, _ = master.all_in_one(sp1, sp2, rhs, [0.3, 0.4, 0.3])
    cell = master.sdCell(sp1, None)
    epi = SimpleNamespace(objective_weight=1.0, lower_bound=0.0, total_scenario_weight=10.0,
                          cuts=[twosd.sdCut(400.0, np.array([-20.0, -15.0, -10.0, -12.0]), 8.0, picks=0)],
                          incumbent_cut=twosd.sdCut(330.0, np.array([-12.0, -9.0, -7.0, -8.0]), 10.0, picks=1))
    cell.bind_epigraph(epi)
    cell.x_candidate = x0.copy()
    cell.x_incumbent = x0.copy()
    cell.add_regularization(x0, 0.1)
    return cell, epi, x0


def _fake_reform(scale):
    from sqlp_amd import twosd

    def reform(epi, cuts, M, seed, index_offset=0):
        B, H = M + 1, len(cuts)
        a = np.zeros((B, H)); b = np.zeros((B, H, 4)); wm = np.zeros((B, H)); tw = np.zeros(B)
        for r in range(B):
            f = 1.0 + scale * r
            tw[r] = epi.total_scenario_weight * f
            for j, c in enumerate(cuts):
                a[r, j], b[r, j], wm[r, j] = c.alpha * f, c.beta * f, c.weight_mark * f
        return twosd.ReformedCuts(a, b, wm, tw)
    return reform


def test_gap_test_arithmetic_without_a_device():
    from sqlp_amd import stopping, twosd
    cell, epi, x0 = _hand_cell()
    res = stopping.bootstrap_gap_test(cell, M=4, seed=1, reform=_fake_reform(0.01))
    assert res.U.shape == res.L.shape == res.gaps.shape == (5,)
    assert res.gaps[0] >= 0.0
    # the identity replicate is the cell's own master
    cell.sync_cuts()
    cell.solve_master()
    U = cell.objf_original(x0) + twosd.evaluate_multi_epigraph(cell.epi, x0)
    assert res.U[0] == pytest.approx(U, rel=1e-12)
    assert res.L[0] == pytest.approx(cell.master_obj, rel=1e-9)
    assert res.gaps[0] == pytest.approx(U - cell.master_obj, rel=1e-6, abs=1e-7)
    epi_r, alpha, beta, _ = cell.cuts.rows()
    np.testing.assert_array_equal(res.rows0[0], epi_r)
    np.testing.assert_allclose(res.rows0[1], alpha, rtol=1e-14)
    np.testing.assert_allclose(res.rows0[2], beta, rtol=1e-14)
    # fraction and passed follow the definition
    thr = 1e-3 * (1 + abs(res.U[0]))
    assert res.threshold == thr
    assert res.fraction == np.count_nonzero(res.gaps[1:] <= thr) / 4
    assert res.passed == (res.fraction >= 0.95)
    # replicates scaled by 1 + 0.01 b scale both estimates' epigraph part alike: U_b - c'x grows with b
    assert np.all(np.diff(res.U) > 0)


def test_gap_test_refuses_cuts_without_picks():
    from sqlp_amd import stopping
    cell, epi, _ = _hand_cell()
    epi.cuts[0].picks = None
    with pytest.raises(ValueError, match="cut 0 of epigraph 0 carries no picks"):
        stopping.bootstrap_gap_test(cell, M=2, reform=_fake_reform(0.0))
    with pytest.raises(ValueError, match="M must be at least 1"):
        stopping.bootstrap_gap_test(cell, M=0, reform=_fake_reform(0.0))
