"""Host side of the mean-CVaR stopping rule (no GPU): risk.bootstrap_gap_test's arithmetic on a
hand-made RiskCell with an injected re-formation, after the pattern of tests/test_boot_host.py.

The cell: lands' root stage, MeanCVaR(0.8, 0.5), one mean cut and one tail row aged 8 of 10, and the
incumbent rows.  The injected reform scales row b of every cut (alpha, beta, weight_mark) and the
total weight by 1 + 0.01 b, so row 0 is the cell's own master."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import instances as I


def _hand_cell():
    from sqlp_amd import master, risk, smps, twosd
    inst = I.load("lands")
    sp1 = smps.get_smps_stage_template(inst["cor"], inst["tim"], 1)
    sp2 = inst["sp2"]
    row = sp2.stage_constraints.index("S2C5")
    rhs = []
    for v in (3.0, 5.0, 7.0):
        r = sp2.r.copy(); r[row] = v; rhs.append(r)
    _, x0, _ = master.all_in_one(sp1, sp2, rhs, [0.3, 0.4, 0.3])
    cell = risk.RiskCell(sp1, None, risk.MeanCVaR(0.8, 0.5))
    epi = SimpleNamespace(objective_weight=1.0, lower_bound=0.0, total_scenario_weight=10.0,
                          cuts=[twosd.sdCut(400.0, np.array([-20.0, -15.0, -10.0, -12.0]), 8.0, picks=0)],
                          incumbent_cut=twosd.sdCut(330.0, np.array([-12.0, -9.0, -7.0, -8.0]), 10.0, picks=1))
    cell.bind_epigraph(epi)
    eta0 = 150.0
    # tail cuts of those two cuts: a quarter / a fifth of their weight scores above eta
    t_old = twosd.sdTailCut(520.0, np.array([-26.0, -19.0, -13.0, -15.0]), 2.0, 8.0, eta0, picks=2)
    t_inc = twosd.sdTailCut(450.0, np.array([-17.0, -12.0, -9.0, -11.0]), 2.0, 10.0, eta0, picks=3)
    cell.tail_cuts.append(risk.tail_row(t_old, 8.0))
    cell.tail_incumbent = risk.tail_row(t_inc, 10.0)
    cell.x_candidate = x0.copy()
    cell.x_incumbent = x0.copy()
    cell.eta_candidate = cell.eta_incumbent = eta0
    cell.add_regularization(x0, eta0, 0.1)
    return cell, epi, x0, eta0


def _fake_reform(scale, zero_inc=()):
    """Row b = the cuts scaled by 1 + scale b; the replicates in zero_inc drew no scenario of the
    incumbent cut (column 1): the zero cut with weight_mark 0 there."""
    from sqlp_amd import twosd

    def reform(epi, cuts, M, seed, index_offset=0):
        B, H = M + 1, len(cuts)
        a = np.zeros((B, H)); b = np.zeros((B, H, 4)); wm = np.zeros((B, H)); tw = np.zeros(B)
        for r in range(B):
            f = 1.0 + scale * r
            tw[r] = epi.total_scenario_weight * f
            for j, c in enumerate(cuts):
                if j == 1 and r in zero_inc:
                    continue
                a[r, j], b[r, j], wm[r, j] = c.alpha * f, np.asarray(c.beta) * f, c.weight_mark * f
        reform.cuts = cuts
        return twosd.ReformedCuts(a, b, wm, tw)
    return reform


def test_tail_row_carries_the_handle_and_is_undone():
    from sqlp_amd import risk, twosd
    t = twosd.sdTailCut(520.0, np.array([-26.0, -19.0, -13.0, -15.0]), 2.0, 8.0, 150.0, picks=7)
    row = risk.tail_row(t, 8.0)
    assert row.picks == 7 and row.weight_mark == 8.0
    back = risk._tail_of_row(row)
    assert back.picks == 7 and back.weight_mark == 2.0
    assert back.alpha == pytest.approx(520.0, rel=1e-15)
    np.testing.assert_allclose(back.beta, t.beta, rtol=1e-15)
    empty = risk._tail_of_row(risk.tail_row(twosd.sdTailCut(0.0, np.zeros(4), 0.0, 8.0, 150.0, picks=8), 8.0))
    assert empty.alpha == 0.0 and not empty.beta.any() and empty.weight_mark == 0.0 and empty.picks == 8


def test_gap_test_arithmetic_without_a_device():
    from sqlp_amd import risk, stopping, twosd
    cell, epi, x0, eta0 = _hand_cell()
    fake = _fake_reform(0.01)
    res = risk.bootstrap_gap_test(cell, M=4, seed=1, reform=fake)
    assert isinstance(res, stopping.GapTest)
    assert res.U.shape == res.L.shape == res.gaps.shape == (5,)
    # one call over the mean cut, the incumbent cut, the tail handle and the incumbent tail
    assert [c.picks for c in fake.cuts] == [0, 1, 2, 3]
    # row 0 is the cell's own master
    var, alpha, beta = cell.master_rows()
    np.testing.assert_array_equal(res.rows0[0], var)
    np.testing.assert_allclose(res.rows0[1], alpha, rtol=1e-14)
    np.testing.assert_allclose(res.rows0[2], beta, rtol=1e-14)
    assert len(res.rows) == 5 and res.rows[0] is res.rows0
    # the identity replicate
    U = cell.objf_original(x0, eta0) + twosd.evaluate_multi_epigraph(cell.composite(), np.append(x0, eta0))
    assert res.U[0] == pytest.approx(U, rel=1e-12)
    cell.solve_master()
    assert res.L[0] == pytest.approx(cell.master_obj, rel=1e-9)
    assert res.gaps[0] >= 0.0
    # fraction and passed follow the definition
    thr = 1e-3 * (1 + abs(res.U[0]))
    assert res.threshold == thr
    assert res.fraction == np.count_nonzero(res.gaps[1:] <= thr) / 4
    assert res.passed == (res.fraction >= 0.95)
    # the discounts are ratios of weights scaled alike: every row grows with 1 + 0.01 b
    for b in (1, 4):
        np.testing.assert_array_equal(res.rows[b][0], var)
        np.testing.assert_allclose(res.rows[b][1], alpha * (1 + 0.01 * b), rtol=1e-13)
        # the eta coefficient is the discount itself: unchanged
        np.testing.assert_allclose(res.rows[b][2][:, :4], beta[:, :4] * (1 + 0.01 * b), rtol=1e-13)
        np.testing.assert_allclose(res.rows[b][2][:, 4], beta[:, 4], rtol=1e-13)


def test_solve_master_rows_changes_nothing():
    cell, epi, x0, eta0 = _hand_cell()
    var, alpha, beta = cell.master_rows()
    res, lam, obj = cell.solve_master_rows(var, alpha, beta)
    assert res.status == "OPTIMAL" and lam.shape == (len(alpha),)
    assert cell.master_status is None and cell.master_obj is None and cell._mean_duals is None
    x, eta = cell.solve_master()
    assert cell.master_obj == obj and np.array_equal(x, res.z[:4]) and eta == res.z[4]
    np.testing.assert_array_equal(cell._mean_duals, lam[:1])
    np.testing.assert_array_equal(cell._tail_duals, lam[2:3])


def test_replicate_without_the_incumbent_cut():
    """W_inc,b = 0: the incumbent mean row is the lower bound, the incumbent tail row is dropped,
    tau >= 0 stays (the master is solved)."""
    from sqlp_amd import risk
    cell, epi, x0, eta0 = _hand_cell()
    res = risk.bootstrap_gap_test(cell, M=3, seed=1, reform=_fake_reform(0.01, zero_inc={2}))
    var, alpha, beta = res.rows[2]
    np.testing.assert_array_equal(var, [0, 0, 1])          # mean cut, the bound in place of the incumbent, one tail row
    assert alpha[1] == epi.lower_bound and not beta[1].any()
    assert len(res.rows[1][0]) == len(res.rows[3][0]) == 4
    assert np.isfinite(res.L[2]) and res.gaps[2] >= -1e-9 * (1 + abs(res.U[2]))
    # with every tail row below 0 at the incumbent the tail estimate is the floor 0
    z = np.append(x0, eta0 + 1e4)
    cell.eta_incumbent = eta0 + 1e4
    far = risk.bootstrap_gap_test(cell, M=1, seed=1, reform=_fake_reform(0.0))
    v0, a0, b0 = far.rows0
    assert ((a0 + b0 @ z)[v0 == 1] < 0.0).all()
    wm, wt = cell.weights()
    mean_at = max(epi.lower_bound, float((a0 + b0 @ z)[v0 == 0].max()))
    assert far.U[0] == pytest.approx(cell.objf_original(x0, eta0 + 1e4) + wm * mean_at, rel=1e-14)


def test_refusals():
    from sqlp_amd import risk
    cell, epi, x0, eta0 = _hand_cell()
    with pytest.raises(ValueError, match="M must be at least 1"):
        risk.bootstrap_gap_test(cell, M=0, reform=_fake_reform(0.0))
    cell.tail_cuts[0].picks = None
    with pytest.raises(ValueError, match="tail row 0 carries no picks"):
        risk.bootstrap_gap_test(cell, M=2, reform=_fake_reform(0.0))
    cell, epi, x0, eta0 = _hand_cell()
    cell.tail_incumbent.picks = None
    with pytest.raises(ValueError, match="incumbent tail row carries no picks"):
        risk.bootstrap_gap_test(cell, M=2, reform=_fake_reform(0.0))
    cell, epi, x0, eta0 = _hand_cell()
    epi.cuts[0].picks = None
    with pytest.raises(ValueError, match="cut 0 of epigraph 0 carries no picks"):
        risk.bootstrap_gap_test(cell, M=2, reform=_fake_reform(0.0))
    # sd_run keeps its refusal and points to the loop that has the rule
    with pytest.raises(TypeError, match="sd_run_stop"):
        risk.sd_run(cell, lambda i: [], 1, stop=lambda c: None)
    with pytest.raises(ValueError, match="check_every"):
        risk.sd_run_stop(cell, lambda i: [], 1, check_every=0)


def test_lam_zero_delegates_to_the_risk_neutral_test():
    from sqlp_amd import risk, stopping
    cell, epi, x0, eta0 = _hand_cell()
    flat = risk.RiskCell(cell.cell.sp1, None, risk.MeanCVaR(0.8, 0.0))
    flat.bind_epigraph(epi)
    flat.x_candidate, flat.x_incumbent = x0.copy(), x0.copy()
    flat.cell.add_regularization(x0, 0.1)
    a = risk.bootstrap_gap_test(flat, M=3, seed=2, reform=_fake_reform(0.01))
    b = stopping.bootstrap_gap_test(flat.cell, M=3, seed=2, reform=_fake_reform(0.01))
    np.testing.assert_array_equal(a.U, b.U)
    np.testing.assert_array_equal(a.L, b.L)
