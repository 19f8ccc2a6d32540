"""The mean-CVaR SD loop (sqlp_amd/risk.py) on data/smps/lands3b: level 0.8, lam 0.5, seeds
11 / 12 / 13, 60 iterations from lands' x_EV, one scenario per iteration drawn from the six joint
realisations (the 0.2 tail spans several of them).

After a run:
* every mean row and every tail row of the final master, aged, bounds the corresponding empirical
  function of the drawn sample from below -- (1/N) sum h(x, w_s) and (1/N) sum (h(x, w_s) - eta)+,
  h by HiGHS -- at the incumbent, at the candidate and at two further (x, eta) points, to the
  project's cut tolerance 1e-8 (1 + |ref|);
* the true composite objective of the final incumbent x (enumerated over the support with HiGHS,
  eta re-optimised exactly: the level-quantile of the six values) is at least the extensive
  mean-CVaR optimum - 1e-6 (an LP with one u_s >= h_s - eta row per realisation, HiGHS);
* its relative gap to that optimum is at most 5 G0, where G0 is the worst relative gap over the
  same three seeds of the risk-neutral master.sd_run on lands3b at 60 iterations, measured on the
  parent commit (profiles/risk/README.md), and 5 = 1 / (1 - level) is the weight the objective puts
  on each tail observation.

lam = 0: risk.sd_run gives the x iterates of master.sd_run, array_equal."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import instances as I

pytestmark = pytest.mark.gpu

LEVEL, LAM, ITERS, SEEDS = 0.8, 0.5, 60, (11, 12, 13)
# worst relative gap of the risk-neutral loop over SEEDS at ITERS iterations on the parent commit
# (profiles/risk/README.md: the three gaps, the command, and the risk gaps measured beside them)
G0 = 1.2623929172679946e-03


@functools.lru_cache(maxsize=None)
def lands3b():
    from oracle import smps_ref
    from sqlp_amd import smps
    cor, tim, sto = smps.load_smps(os.path.join(I.DATA, "lands3b"))
    sp1 = smps.get_smps_stage_template(cor, tim, 1)
    sp2 = smps.get_smps_stage_template(cor, tim, 2)
    positions, rows, cols = smps.scenario_positions(sp2, sto)
    support, probs = smps.joint_support(sto, positions)
    inst = I.load("lands")                                 # the same core file: the oracle's templates
    return SimpleNamespace(sto=sto, sp1=sp1, sp2=sp2, rows=rows, support=np.asarray(support), probs=np.asarray(probs) / np.sum(probs),
                           osp1=inst["osp1"], osp2=inst["osp2"], x_ev=I.x_ev("lands"))


def draws(seed, n=ITERS):
    L = lands3b()
    return np.random.default_rng(seed).choice(len(L.probs), size=n, p=L.probs)


def recourse(x, values):
    """h(x, w) of every row of values (HiGHS on the oracle's template)."""
    from oracle import lp_highs
    L = lands3b()
    sp = L.osp2
    out = []
    for v in values:
        b = sp.r - sp.T @ np.asarray(x)
        b[L.rows] += v - sp.r[L.rows]
        st, o, _, _ = lp_highs.solve_rhs(sp, b)
        assert st == 0, (x, v, st)
        out.append(o)
    return np.array(out)


def quantile(h, p, level):
    """The smallest value with cumulative probability >= level (to 1e-12)."""
    order = np.argsort(h)
    cum = np.cumsum(p[order])
    return float(h[order][np.searchsorted(cum, level - 1e-12)])


def true_objective(x, lam, level=LEVEL):
    """c'x + (1 - lam) E h + lam CVaR_level(h) over the support, eta at the exact quantile."""
    L = lands3b()
    h = recourse(x, L.support)
    eta = quantile(h, L.probs, level)
    return float(L.osp1.q @ x) + (1 - lam) * float(L.probs @ h) + lam * (eta + float(L.probs @ np.maximum(h - eta, 0.0)) / (1 - level))


@functools.lru_cache(maxsize=None)
def extensive_optimum(lam, level=LEVEL):
    """HiGHS on min c'x + sum_s p_s ((1 - lam) q'y_s + lam u_s / (1 - level)) + lam eta over x (stage-1
    rows and bounds), eta free, y_s >= 0 with T x + W y_s (sense) r_s, u_s >= q'y_s - eta, u_s >= 0."""
    from scipy.optimize import linprog
    from oracle.lp_highs import _split
    L = lands3b()
    sp1, sp2 = L.osp1, L.osp2
    S = len(L.probs)
    m1, n1 = sp1.W.shape
    m2, n2 = sp2.W.shape
    nz = n1 + 1 + S * (n2 + 1)                              # x, eta, (y_s, u_s)
    A = np.zeros((m1 + S * m2, nz))
    A[:m1, :n1] = sp1.W
    rhs = [sp1.r]
    c = np.zeros(nz)
    c[:n1] = sp1.q
    c[n1] = lam
    U = np.zeros((S, nz))
    for s in range(S):
        o = n1 + 1 + s * (n2 + 1)
        A[m1 + s * m2:m1 + (s + 1) * m2, :n1] = sp2.T
        A[m1 + s * m2:m1 + (s + 1) * m2, o:o + n2] = sp2.W
        r = sp2.r.copy()
        r[L.rows] = L.support[s]
        rhs.append(r)
        c[o:o + n2] = (1 - lam) * L.probs[s] * sp2.q
        c[o + n2] = lam * L.probs[s] / (1 - level)
        U[s, o:o + n2] = sp2.q                             # q'y_s - eta - u_s <= 0
        U[s, n1] = -1.0
        U[s, o + n2] = -1.0
    _, _, _, A_ub, b_ub, A_eq, b_eq = _split(list(sp1.senses) + list(sp2.senses) * S, A, np.concatenate(rhs))
    A_ub = np.vstack([A_ub, U]) if A_ub is not None and len(A_ub) else U
    b_ub = np.concatenate([b_ub, np.zeros(S)]) if b_ub is not None and len(b_ub) else np.zeros(S)
    bounds = [(None if np.isinf(l) else l, None if np.isinf(u) else u) for l, u in zip(sp1.cur_lb, sp1.cur_ub)] + [(None, None)]
    bounds += ([(0, None)] * (n2 + 1)) * S
    res = linprog(c, A_ub=A_ub, b_ub=b_ub, A_eq=A_eq if A_eq is not None and len(A_eq) else None,
                  b_eq=b_eq if b_eq is not None and len(b_eq) else None, bounds=bounds, method="highs")
    assert res.status == 0, res.message
    return float(res.fun)


def risk_cell(lam):
    from sqlp_amd import risk, smps, twosd
    L = lands3b()
    ctx = twosd.SDContext(L.sp2, L.sto)
    ctx.compute_basis(L.x_ev, smps.mean_values(L.sto))
    cell = risk.RiskCell(L.sp1, ctx, risk.MeanCVaR(LEVEL, lam))
    cell.bind_epigraph(twosd.sdEpigraph(ctx, 1.0, 0.0))
    cell.x_candidate = L.x_ev.copy()
    cell.x_incumbent = L.x_ev.copy()
    return ctx, cell


def run_risk(seed, lam=LAM, iters=ITERS):
    from sqlp_amd import risk
    L = lands3b()
    ctx, cell = risk_cell(lam)
    d = draws(seed, iters)
    assert risk.sd_run(cell, lambda i: [L.support[d[i]][None, :]], iters) == iters
    return ctx, cell, d


def relative_gap(x, lam):
    opt = extensive_optimum(lam)
    true = true_objective(x, lam)
    return true, opt, (true - opt) / abs(opt)


@pytest.mark.parametrize("seed", SEEDS)
def test_mean_cvar_loop_on_lands3b(seed):
    L = lands3b()
    ctx, cell, d = run_risk(seed)
    x, eta = cell.x_incumbent, cell.eta_incumbent
    sample = L.support[d]
    var, alpha, beta = cell.master_rows()
    assert (var == 0).sum() >= 2 and (var == 1).sum() >= 2
    points = [(x, eta), (cell.x_candidate, cell.eta_candidate), (1.1 * x, eta - 25.0), (x + np.array([0.5, 0.0, 0.5, 0.0]), eta + 30.0)]
    worst = -np.inf
    for xp, ep in points:
        h = recourse(xp, L.support)[d]                      # h of every drawn scenario
        ref = (float(h.mean()), float(np.maximum(h - ep, 0.0).mean()))
        z = np.append(xp, ep)
        for v, a, b in zip(var, alpha, beta):
            row = a + float(b @ z)
            worst = max(worst, (row - ref[v]) / (1 + abs(ref[v])))
            assert row <= ref[v] + 1e-8 * (1 + abs(ref[v])), (seed, v, row, ref[v], xp, ep)
    true, opt, gap = relative_gap(x, LAM)
    print(f"RISK loop lands3b seed {seed}: objective at the incumbent {true:.6f}, extensive mean-CVaR optimum {opt:.6f}, "
          f"relative gap {gap:.6e}, eta {eta:.4f}, {len(alpha)} rows, worst row excess {worst:.2e} (relative)")
    assert true >= opt - 1e-6
    assert gap <= 5.0 * G0, (seed, gap, G0)                 # 5 = 1 / (1 - level); G0: profiles/risk/README.md
    ctx.close()


def test_lam_zero_is_the_risk_neutral_loop():
    from sqlp_amd import master, risk, smps, twosd
    L = lands3b()
    iters, d = 30, draws(11, 30)
    xs_r, xs_m = [], []
    ctx, cell = risk_cell(0.0)

    def nxt_r(i):
        xs_r.append(cell.x_candidate.copy())
        return [L.support[d[i]][None, :]]

    risk.sd_run(cell, nxt_r, iters)
    xs_r.append(cell.x_candidate.copy())
    ctx.close()
    ctx2 = twosd.SDContext(L.sp2, L.sto)
    ctx2.compute_basis(L.x_ev, smps.mean_values(L.sto))
    mc = master.sdCell(L.sp1, ctx2)
    mc.bind_epigraph(twosd.sdEpigraph(ctx2, 1.0, 0.0))
    mc.x_candidate, mc.x_incumbent = L.x_ev.copy(), L.x_ev.copy()

    def nxt_m(i):
        xs_m.append(mc.x_candidate.copy())
        return [L.support[d[i]][None, :]]

    master.sd_run(mc, nxt_m, iters, min_iter=10 ** 9, stop=lambda c: SimpleNamespace(passed=False))
    xs_m.append(mc.x_candidate.copy())
    np.testing.assert_array_equal(np.array(xs_r), np.array(xs_m))
    np.testing.assert_array_equal(cell.x_incumbent, mc.x_incumbent)
    ctx2.close()
