"""Farkas rays of infeasible stage-2 LPs: the LP kernel's ray instantiation through twosd_solve_rays
(DESIGN.md §5.12), on lands3f and on the generated incomplete-recourse template at the 64-row slot
boundaries, with and without bound rows, with k in one and in two 64-slices and random T elements
(tests/feas_cases.py).

References: HiGHS (oracle/lp_highs.py, status 2) and the C dual simplex (ST_INFEASIBLE) for the
infeasible set; numpy.linalg.solve on the returned basis head and leaving row for the ray itself,
to 1e-9 of max |sigma| (the tolerance tests/test_gpu_lp.py uses against the oracle); the ratio
test's pivot tolerance HTOL_PIV = 1e-9 plus a rounding term for sigma' W_j <= 0."""
import ctypes as C

import numpy as np
import pytest

from tests import feas_cases as FC

pytestmark = pytest.mark.gpu

HTOL_PIV = 1e-9
EPS = np.finfo(np.float64).eps


def _check_rays(W, sense, B, rb, first=0):
    """Every returned ray against the canonical LP (W: m x n, sense, B: the scenarios' rhs rows)."""
    m, n = W.shape
    sense = np.array(list(sense))
    assert len(rb.scen) == len(rb.rays) == len(rb.row) == len(rb.head)
    assert (np.diff(rb.scen) > 0).all()                                   # scenario order
    worst = 0.0
    for s, sig, r, head in zip(rb.scen, rb.rays, rb.row, rb.head):
        assert rb.status[s - first] == 1
        assert np.isfinite(sig).all() and np.abs(sig).max() > 0
        assert (sig[sense == "G"] >= 0).all() and (sig[sense == "L"] <= 0).all()
        lim = HTOL_PIV + 4 * EPS * (np.abs(sig)[:, None] * np.abs(W)).sum(axis=0)
        assert (sig @ W <= lim).all(), (s, float((sig @ W - lim).max()))
        assert sig @ B[s - first] > 0, (s, float(sig @ B[s - first]))
        # sigma = +-e_r' B^{-1}
        assert 0 <= r < m and sorted(set(head.tolist())) == sorted(head.tolist())
        Bm = np.zeros((m, m))
        for i, j in enumerate(head):
            if j < n:
                Bm[:, i] = W[:, j]
            else:
                Bm[j - n, i] = 1.0
        rho = np.linalg.solve(Bm.T, np.eye(m)[r])
        err = min(np.abs(sig - rho).max(), np.abs(sig + rho).max())
        worst = max(worst, err / np.abs(sig).max())
        assert err <= 1e-9 * np.abs(sig).max(), (s, err)
    return worst


def _retries(ctx):
    e, r = C.c_int64(), C.c_int64()
    from sqlp_amd._lib import check
    check(ctx.lib.twosd_last_lp_eta_entries(ctx.h, C.byref(e), C.byref(r)))
    return r.value


def _oracle(S, x, vals):
    """(C-oracle LP on the canonical form started from the slack basis' optimum of scenario 0, its
    head, statuses, pivots) at x."""
    from oracle import cpu
    K = S.canon
    lp = cpu.CpuLP(K.W, K.q, K.sense)
    B = FC.rhs_lp(S, x, vals)
    st0, _, head, _ = lp.solve_from_slack(B[0])
    assert st0 == 0 and lp.set_basis(head) <= 1e-9
    base = B[0].copy()
    base[S.rows] -= FC.deltas(S, x, vals[:1])[0]           # scenario 0 is the template: its deltas are zero anyway
    _, _, _, ost, it = lp.solve_batch(S.rows, base, FC.deltas(S, x, vals), kmax=512)
    return head, ost, it, B


def _context(S, head):
    from sqlp_amd import twosd
    ctx = twosd.SDContext(S.sp2, positions=S.positions)
    assert (ctx.m_lp, ctx.k) == (S.m_lp, S.k)
    np.testing.assert_array_equal(ctx.rows, S.rows)
    np.testing.assert_array_equal(ctx.cols, S.cols)
    ctx.set_basis(head)
    return ctx


@pytest.mark.parametrize("cid", list(FC.CASES))
def test_rays_on_the_generated_template(cid):
    from sqlp_amd import twosd
    S = FC.incomplete(cid)
    vals = FC.values(S)
    N = len(vals)
    x = FC.X0
    head, ost, oit, B = _oracle(S, x, vals)
    hst = FC.highs_status(S, x, vals)
    ctx = _context(S, head)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals)
    rb = twosd.solve_rays(epi, x, 0, N, cap=256, push=False)
    inf = np.flatnonzero(rb.status == 1)
    np.testing.assert_array_equal(inf, np.flatnonzero(hst == 2))
    np.testing.assert_array_equal(inf, np.flatnonzero(ost == 1))
    assert set(np.unique(rb.status)) <= {0, 1} and rb.n_infeasible == len(inf) > 0
    assert 0 < len(rb.scen) <= len(inf) and rb.scen[0] == inf[0]
    assert twosd.sdFeasRaySet(ctx).size == 0                              # push=False
    worst = _check_rays(S.canon.W, S.canon.sense, B, rb)
    its, _ = ctx.last_lp_iters(N)
    print(f"FEAS rays {cid}: {len(inf)} infeasible, {len(rb.scen)} rays, exits at K = 0: {(its[inf] == 0).sum()}, "
          f"K > 0: {(its[inf] > 0).sum()}, worst |sigma -+ e_r'B^-1| / max|sigma| = {worst:.2e}")
    if cid == "m5b":
        assert (its[inf] == 0).any()                                      # an exit at K = 0
    if cid == "m65":
        assert (its[inf] > 0).any()                                       # an exit at K > 0
    # cap below the number of distinct rays: truncated in scenario order
    if len(rb.scen) >= 2:
        cap = len(rb.scen) - 1
        rc = twosd.solve_rays(epi, x, 0, N, cap=cap, push=False)
        assert rc.n_infeasible == len(inf)
        np.testing.assert_array_equal(rc.scen, rb.scen[:cap])
        np.testing.assert_array_equal(rc.rays, rb.rays[:cap])
    # push=True leaves F equal to pushing the returned rays by hand
    F = twosd.sdFeasRaySet(ctx)
    rp = twosd.solve_rays(epi, x, 0, N, cap=256, push=True)
    np.testing.assert_array_equal(rp.rays, rb.rays)
    pushed = F.get()
    F.clear()
    assert F.size == 0
    idx = F.push_batch(rb.rays)
    assert idx.max() + 1 == F.size == len(pushed)
    np.testing.assert_array_equal(F.get(), pushed)
    for ray, i in zip(rb.rays, idx):
        np.testing.assert_array_equal(twosd.fray_key(ray)[1], pushed[i])
    # a second call with F filled: every infeasible scenario is cut off by a held ray, none is re-solved
    r2 = twosd.solve_rays(epi, x, 0, N, cap=256, push=True)
    assert r2.n_infeasible == len(inf) and len(r2.scen) == 0 and F.size == len(pushed)
    assert twosd.last_ray_stats(ctx) == (0, len(inf))
    # a batch with no infeasible scenario: what solve_batch reports
    feas = np.flatnonzero(hst == 0)
    e2 = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(e2, vals[feas])
    r0 = twosd.solve_rays(e2, x, 0, len(feas), cap=8, push=True)
    _, _, _, st = twosd.solve_batch(e2, x, 0, len(feas), want_pi=False)
    assert r0.n_infeasible == 0 and len(r0.scen) == 0
    np.testing.assert_array_equal(r0.status, st)
    assert (st == 0).all()
    ctx.close()


def test_rays_with_a_pool_of_three_bases_and_a_retry():
    """An infeasible scenario whose pool start is not the primary basis is retried from the
    primary basis; the ray is that of the retry."""
    from sqlp_amd import twosd
    S = FC.incomplete("m65")
    vals = FC.values(S)
    N = len(vals)
    x = FC.X0
    head, ost, _, B = _oracle(S, x, vals)
    ctx = _context(S, head)
    feas = np.flatnonzero(ost == 0)
    tr = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(tr, vals[feas])
    assert ctx.pool_build(tr, x, 0, len(feas), 3) == 3 == ctx.pool_size()
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals)
    rb = twosd.solve_rays(epi, x, 0, N, cap=256, push=False)
    retries = _retries(ctx)
    np.testing.assert_array_equal(np.flatnonzero(rb.status == 1), np.flatnonzero(ost == 1))
    print(f"FEAS rays pool: {rb.n_infeasible} infeasible, {retries} pool starts retried from the primary basis")
    assert retries > 0
    assert (ctx.last_pool_picks(N)[rb.status == 1] == 0).all()            # a retried start is recorded as the primary
    _check_rays(S.canon.W, S.canon.sense, B, rb)
    ctx.close()


def test_rays_on_lands3f_at_x_ev():
    from oracle import cpu, lp_highs
    from sqlp_amd import smps, twosd
    L = FC.lands3f()
    sp = L.osp2
    x = L.x_ev
    ctx = twosd.SDContext(L.sp2, L.sto)
    assert ctx.k == 3 and [p.row_name for p in ctx.positions] == list(FC.LANDS3F_ROWS)
    ctx.compute_basis(x, smps.mean_values(L.sto))
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, L.support)
    B = FC.lands3f_rhs(L, x, L.support)
    hst = np.array([lp_highs.solve_rhs(sp, b)[0] for b in B])
    lp = cpu.CpuLP(sp.W, sp.q, sp.senses)
    lp.set_basis(ctx.get_basis())
    rows = np.array([sp.row_names.index(r) for r in FC.LANDS3F_ROWS], dtype=np.int32)
    _, _, _, ost, _ = lp.solve_batch(rows, sp.r - sp.T @ x, L.support - sp.r[rows])
    rb = twosd.solve_rays(epi, x, 0, 6, cap=16, push=True)
    np.testing.assert_array_equal(np.flatnonzero(rb.status == 1), FC.LANDS3F_INFEASIBLE)
    np.testing.assert_array_equal(np.flatnonzero(hst == 2), FC.LANDS3F_INFEASIBLE)
    np.testing.assert_array_equal(np.flatnonzero(ost == 1), FC.LANDS3F_INFEASIBLE)
    assert rb.n_infeasible == 2 and 1 <= len(rb.scen) <= 2 and rb.scen[0] == 4
    _check_rays(sp.W, sp.senses, B, rb)
    assert twosd.sdFeasRaySet(ctx).size == len(rb.scen)
    # the four feasible points solve as before
    obj, _, _, st = twosd.solve_batch(epi, x, 0, 4, want_pi=False)
    assert (st == 0).all()
    np.testing.assert_allclose(obj, FC.LANDS3F_RECOURSE, atol=1e-4)
    # a ray of lands at x_EV says: total demand exceeds total capacity
    print("lands3f rays:", np.round(rb.rays, 6).tolist(), "rows", rb.row.tolist())
    ctx.close()
