"""SD on instances without relatively complete recourse: sd_run with
feasibility=True on lands3f and on the generated incomplete-recourse template, against HiGHS on the
CPU: every stored feasibility row is valid for the set of x at which all support LPs are feasible,
the final incumbent lies in that set, and its true objective is bounded below by the extensive
optimum.  With feasibility=False the first infeasible draw raises, as before.

Measured on lands3f (60 iterations from x_EV, seed 11): the figures are printed here and recorded
in profiles/feas/README.md; the gap to the extensive optimum is not asserted."""
import numpy as np
import pytest

from tests import feas_cases as FC

pytestmark = pytest.mark.gpu

ITERS_A, SEED_A = 60, 11


def _draws(probs, n, seed):
    return np.random.default_rng(seed).choice(len(probs), size=n, p=probs)


def _lands_cell():
    from sqlp_amd import master, smps, twosd
    L = FC.lands3f()
    ctx = twosd.SDContext(L.sp2, L.sto)
    ctx.compute_basis(L.x_ev, smps.mean_values(L.sto))
    cell = master.sdCell(L.sp1, ctx)
    cell.bind_epigraph(twosd.sdEpigraph(ctx, 1.0, 0.0))
    cell.x_candidate = L.x_ev.copy()
    cell.x_incumbent = L.x_ev.copy()
    return L, ctx, cell


def _never(cell):
    from types import SimpleNamespace
    return SimpleNamespace(passed=False)


def _support_status(ctx, x, support):
    from sqlp_amd import twosd
    e = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(e, support)
    return twosd.solve_rays(e, x, 0, len(support), cap=0, push=False).status


def test_sd_run_on_lands3f_with_feasibility_rows():
    from oracle import lp_highs
    from sqlp_amd import master
    L, ctx, cell = _lands_cell()
    draws = _draws(L.probs, ITERS_A, SEED_A)
    assert (draws == 5).any()                                             # the point with total demand 14 is drawn
    it, _ = master.sd_run(cell, lambda i: [L.support[draws[i]][None, :]], ITERS_A, min_iter=10 ** 9, stop=_never, feasibility=True)
    assert it == ITERS_A
    x = cell.x_incumbent
    margin = master.DEFAULT_FEAS_MARGIN
    assert x.sum() >= FC.LANDS3F_MIN_CAPACITY - margin, x.sum()
    np.testing.assert_array_equal(_support_status(ctx, x, L.support), 0)  # all six support LPs optimal
    assert len(cell.feas_rows) >= 1
    sp1, sp2 = L.osp1, L.osp2
    rows = [sp2.row_names.index(r) for r in FC.LANDS3F_ROWS]
    rs = []
    for v in L.support:
        r = sp2.r.copy()
        r[rows] = v
        rs.append(r)
    Ts = [sp2.T] * 6
    worst = -np.inf
    for a, b in cell.feas_rows:                                           # every stored row is valid
        st, val, _ = FC.extensive_lp(sp1.q, sp1.W, sp1.r, sp1.senses, sp1.cur_lb, sp1.cur_ub, sp2.W, sp2.q, sp2.senses, Ts, rs, L.probs, obj_x=b)
        assert st == 0
        worst = max(worst, (a + val) / (1 + abs(a)))
        assert a + val <= 1e-9 * (1 + abs(a)), (a, b, val)
    true = float(sp1.q @ x)
    for p, r in zip(L.probs, rs):
        st, obj, _, _ = lp_highs.solve_rhs(sp2, r - sp2.T @ x)
        assert st == 0
        true += p * obj
    assert true >= FC.LANDS3F_OPT - 1e-6                                   # the extensive optimum bounds every feasible point
    st, opt, _ = FC.extensive_lp(sp1.q, sp1.W, sp1.r, sp1.senses, sp1.cur_lb, sp1.cur_ub, sp2.W, sp2.q, sp2.senses, Ts, rs, L.probs)
    assert st == 0 and abs(opt - FC.LANDS3F_OPT) <= 1e-5
    print(f"FEAS loop lands3f: {ITERS_A} iterations, sum(x) = {x.sum():.9f}, objective at the incumbent {true:.6f}, extensive optimum "
          f"{opt:.6f}, gap {100 * (true - opt) / opt:.3f} %, {len(cell.feas_rows)} rows, worst row violation {worst:.2e} (relative), "
          f"candidate estimate {cell.improvement_info.candidate_estimation:.4f}")
    ctx.close()


def test_sd_run_on_lands3f_without_feasibility_raises_at_the_first_infeasible_draw():
    from sqlp_amd import master
    from sqlp_amd._lib import TwoSDError
    L, ctx, cell = _lands_cell()
    draws = _draws(L.probs, ITERS_A, SEED_A)
    first_bad = int(np.flatnonzero(np.isin(draws, FC.LANDS3F_INFEASIBLE))[0])
    seen = []

    def nxt(i):
        seen.append(i)
        return [L.support[draws[i]][None, :]]

    with pytest.raises(TwoSDError) as e:
        master.sd_run(cell, nxt, ITERS_A, min_iter=10 ** 9, stop=_never)
    assert e.value.code == -4 and seen[-1] == first_bad
    assert not cell.feas_rows
    ctx.close()


def test_sd_run_on_the_generated_template():
    """m_lp = 65, 20 iterations over an enumerated support of 12 scenarios with random T elements."""
    from oracle import lp_highs
    from sqlp_amd import master, twosd
    S = FC.incomplete("m65")
    support = FC.values(S, FC.LOOP_SUPPORT, seed=3)
    probs = np.full(len(support), 1.0 / len(support))
    assert (FC.highs_status(S, FC.X0, support) == 2).any()                # infeasible at the start
    sp1 = FC.loop_stage1()
    ctx = twosd.SDContext(S.sp2, positions=S.positions)
    ctx.compute_basis(FC.X0, support[0])
    cell = master.sdCell(sp1, ctx)
    cell.bind_epigraph(twosd.sdEpigraph(ctx, 1.0, 0.0))
    cell.x_candidate = FC.X0.copy()
    cell.x_incumbent = FC.X0.copy()
    draws = _draws(probs, 20, 5)
    it, _ = master.sd_run(cell, lambda i: [support[draws[i]][None, :]], 20, min_iter=10 ** 9, stop=_never, feasibility=True)
    assert it == 20 and len(cell.feas_rows) >= 1
    x = cell.x_incumbent
    drawn = np.unique(draws)
    np.testing.assert_array_equal(_support_status(ctx, x, support[drawn]), 0)     # every scenario seen so far
    TR = [FC.scenario_T_r(S, v) for v in support]
    A1, b1 = np.ones((1, FC.N1)), np.array([40.0])
    xlb, xub = np.zeros(FC.N1), np.full(FC.N1, 12.0)
    ext = lambda idx, obj_x=None: FC.extensive_lp(FC.LOOP_C1, A1, b1, ["L"], xlb, xub, S.W, S.q, S.sense, [TR[s][0] for s in idx],
                                                   [TR[s][1] for s in idx], probs[idx] / probs[idx].sum(), obj_x=obj_x)
    worst = -np.inf
    for a, b in cell.feas_rows:                                           # valid for the set the full support defines
        st, val, _ = ext(np.arange(len(support)), obj_x=b)
        assert st == 0
        worst = max(worst, (a + val) / (1 + abs(a)))
        assert a + val <= 1e-9 * (1 + abs(a)), (a, b, val)
    # over the scenarios drawn: the incumbent's objective against their extensive optimum
    st, opt, _ = ext(drawn)
    assert st == 0
    true = float(FC.LOOP_C1 @ x)
    for s in drawn:
        hs, obj, _, _ = lp_highs.solve_rhs(S.hp, TR[s][1] - TR[s][0] @ x)
        assert hs == 0
        true += probs[s] / probs[drawn].sum() * obj
    assert true >= opt - 1e-6
    print(f"FEAS loop m65: objective at the incumbent {true:.6f}, extensive optimum over the drawn support {opt:.6f}, "
          f"{len(cell.feas_rows)} rows, worst row violation {worst:.2e} (relative)")
    ctx.close()
