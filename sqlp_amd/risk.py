"""The mean-CVaR SD loop (the reference optimises the expectation only).

    min  c'x + (1 - lam) E[h(x, w)] + lam ( eta + E[(h(x, w) - eta)+] / (1 - level) )

in the form of Rockafellar and Uryasev: eta is a free first-stage variable costing lam, and the
epigraph of the cell contributes two master epigraph variables,

    mean  m   >= d_j (alpha_j + beta_j'x) + (1 - d_j) lb        weight (1 - lam) w_e
    tail  tau >= a_j dt_j (alpha^t_j + beta^t_j'x - eta),  >= 0  weight lam w_e / (1 - level)

The mean rows are the cuts twosd.sd_iteration_cuts builds today.  A tail row comes from
twosd.cut_tail right after its mean cut, at the same x and the eta of that point:
dt_j = tail_weight / total_weight of that cut, and a_j = N_j / N ages the row as the mean rows age
(valid because (h - eta)+ >= 0).  The master point is (x, eta); the prox term covers both; the
incumbent test is twosd.check_improvement on the two composite epigraph values.

One epigraph per cell: CVaR of a sum of recourse functions does not separate over epigraphs.
lam == 0 delegates to master.sd_iteration on the wrapped sdCell, so the x iterates are those of
the risk-neutral loop bit for bit.  Feasibility rows are out of scope here.

The stopping rule (sd_run_stop, bootstrap_gap_test) is the risk-neutral one on both row sets: with
keep_picks every mean cut keeps its pick handle and every tail row a tail handle (twosd.cut_tail's
keep=: the scenarios above eta and their picks, compacted on the device).  With its tail set and
picks fixed a tail row is linear in the scenario weights, so one twosd.reform_cuts call re-forms all
rows under the Poisson(1) replicates.  The tail set is the one of the row's own (x, eta): at that
point the re-formed row is the replicate's own E_b[(h - eta)+], elsewhere a lower bound of it
(DESIGN.md §5.13, §9).  sd_run keeps its fixed iteration count and its int return.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from . import cut_pool, master, stopping, twosd
from .smps import spStageProblem


@dataclass(frozen=True)
class MeanCVaR:
    """The risk measure (1 - lam) E[.] + lam CVaR_level[.], 0 <= lam <= 1, 0 < level < 1."""
    level: float
    lam: float

    def __post_init__(self):
        if not 0.0 < float(self.level) < 1.0:
            raise ValueError(f"MeanCVaR: level = {self.level} outside (0, 1)")
        if not 0.0 <= float(self.lam) <= 1.0:
            raise ValueError(f"MeanCVaR: lam = {self.lam} outside [0, 1]")

    def value(self, mean, eta, tail):
        """(1 - lam) mean + lam (eta + tail / (1 - level)): the composite of E[h], eta, E[(h - eta)+]."""
        return (1.0 - self.lam) * mean + self.lam * (eta + tail / (1.0 - self.level))


def _extend(cut: twosd.sdCut) -> twosd.sdCut:
    """A mean cut in the master's (x, eta) space: no eta term."""
    return twosd.sdCut(cut.alpha, np.append(cut.beta, 0.0), cut.weight_mark)


def tail_row(tail: twosd.sdTailCut, weight_mark: float) -> twosd.sdCut:
    """tau >= d (alpha + beta'x - eta) as a cut over (x, eta), aged through weight_mark as a mean cut is."""
    d = tail.d
    return twosd.sdCut(d * tail.alpha, np.append(d * tail.beta, -d), float(weight_mark), tail.picks)


def _tail_of_row(row: twosd.sdCut) -> twosd.sdCut:
    """tail_row undone: the tail cut (alpha, beta over x, weight_mark = the tail's weight W_t) behind a
    tail row, carrying the row's tail handle -- what reform_cuts re-forms.  d = 0: the zero cut."""
    d = -float(row.beta[-1])
    if d == 0.0:
        return twosd.sdCut(0.0, np.zeros(len(row.beta) - 1), 0.0, row.picks)
    return twosd.sdCut(row.alpha / d, np.asarray(row.beta[:-1]) / d, d * row.weight_mark, row.picks)


class RiskCell:
    """A master.sdCell (self.cell: stage-1 rows, the epigraph, the dual vertex set, the candidate and
    incumbent x) with the risk measure's own state: eta at the candidate and the incumbent, and the
    tail rows of the epigraph."""

    def __init__(self, sp1: spStageProblem, ctx: twosd.SDContext, risk: MeanCVaR):
        self.cell = master.sdCell(sp1, ctx)
        self.risk = risk
        self.eta_candidate = None         # set from the first cut's quantile
        self.eta_incumbent = None
        self.tail_cuts: list = []         # twosd.sdCut over (x, eta), one per kept mean cut's iteration
        self.tail_incumbent = None
        self.improvement_info = None
        self.master_status = None
        self.master_obj = None
        self.reg_center = None            # (x, eta)
        self.rho = 0.0
        self._mean_duals = self._tail_duals = None

    # the points and the schedule's state live on the wrapped cell
    @property
    def x_candidate(self):
        return self.cell.x_candidate

    @x_candidate.setter
    def x_candidate(self, x):
        self.cell.x_candidate = np.array(x, dtype=np.float64)

    @property
    def x_incumbent(self):
        return self.cell.x_incumbent

    @x_incumbent.setter
    def x_incumbent(self, x):
        self.cell.x_incumbent = np.array(x, dtype=np.float64)

    @property
    def ext(self):
        return self.cell.ext

    @property
    def epi(self):
        return self.cell.epi

    @property
    def dual_vertices(self):
        return self.cell.dual_vertices

    def bind_epigraph(self, epi: twosd.sdEpigraph):
        if self.cell.epi:
            raise ValueError("RiskCell: one epigraph per cell (CVaR does not separate over epigraphs)")
        self.cell.bind_epigraph(epi)

    # ---- the composite objective's two epigraphs, as check_improvement and the master read them
    def weights(self):
        """(mean weight, tail weight) of the epigraph in the master's objective."""
        w = self.cell.epi[0].objective_weight
        return (1.0 - self.risk.lam) * w, self.risk.lam * w / (1.0 - self.risk.level)

    def composite(self):
        """The mean and the tail epigraph over (x, eta) at this moment (copies), with the fields
        twosd.evaluate_multi_epigraph reads."""
        epi = self.cell.epi[0]
        wm, wt = self.weights()
        tw = epi.total_scenario_weight
        mean = SimpleNamespace(objective_weight=wm, cuts=[_extend(c) for c in epi.cuts],
                               incumbent_cut=None if epi.incumbent_cut is None else _extend(epi.incumbent_cut),
                               total_scenario_weight=tw, lower_bound=epi.lower_bound)
        tail = SimpleNamespace(objective_weight=wt, cuts=list(self.tail_cuts), incumbent_cut=self.tail_incumbent,
                               total_scenario_weight=tw, lower_bound=0.0)
        return [mean, tail]

    def objf_original(self, x, eta) -> float:
        """The master objective's first-stage part at (x, eta): c'x + lam eta."""
        return self.cell.objf_original(x) + self.risk.lam * float(eta)

    def add_regularization(self, x0, eta0, rho):
        self.reg_center = np.append(np.asarray(x0, dtype=np.float64), float(eta0))
        self.rho = float(rho)

    def master_rows(self):
        """(variable, alpha, beta) of every cut row var >= alpha + beta'(x, eta) in master order: the
        mean epigraph's (variable 0), then the tail epigraph's (variable 1), each its aged cuts
        followed by its incumbent row -- cut_pool.add_cut_to_master's arithmetic."""
        var, alpha, beta = [], [], []
        for v, e in enumerate(self.composite()):
            pool = cut_pool.sdMasterCuts(1)
            for cut in e.cuts:
                cut_pool.add_cut_to_master(pool, cut, v, cut.weight_mark / e.total_scenario_weight, e.lower_bound)
            if e.incumbent_cut is not None:
                cut_pool.add_cut_to_master(pool, e.incumbent_cut, v, 1.0, e.lower_bound)
            for r in pool._rows:
                var.append(v); alpha.append(r.alpha); beta.append(r.beta)
        n = self.cell.n1 + 1
        return np.array(var, dtype=np.int64), np.array(alpha), np.array(beta).reshape(-1, n)

    def solve_master(self):
        """The regularised master over z = (x, eta, m, tau): returns (x, eta) and stores the cut rows'
        multipliers for the next iteration's cut removal."""
        n1 = self.cell.n1
        var, alpha, beta = self.master_rows()
        res, lam, obj = self.solve_master_rows(var, alpha, beta)
        self.master_status = res.status
        if res.status != master.OPTIMAL:
            raise RuntimeError(f"master not solved: {res.status}")
        nm = len(self.cell.epi[0].cuts)
        n_mean_rows = int(np.sum(var == 0))
        self._mean_duals = lam[:nm]
        self._tail_duals = lam[n_mean_rows:n_mean_rows + len(self.tail_cuts)]
        self.master_obj = obj
        return res.z[:n1].copy(), float(res.z[n1])

    def solve_master_rows(self, var, alpha, beta):
        """The cell's regularised master (root-stage rows and bounds, tau >= 0, prox term of the
        current rho and centre) over the given rows var >= alpha + beta'(x, eta), var 0 the mean and
        1 the tail variable: (QPResult, the rows' multipliers, objective value with the prox constant).
        Changes nothing in the cell; solve_master is this on the cell's own rows (the stopping rule
        passes re-formed ones)."""
        c = self.cell
        n1 = c.n1
        nz = n1 + 3
        var = np.asarray(var, dtype=np.int64)
        alpha = np.asarray(alpha, dtype=np.float64)
        if not np.any(var == 0):
            raise RuntimeError("the epigraph has no cut: the master is unbounded")
        wm, wt = self.weights()
        H = np.zeros(nz)
        g = np.concatenate([c.c1, [self.risk.lam, wm, wt]])
        if self.reg_center is not None and self.rho != 0.0:
            H[:n1 + 1] = self.rho
            g[:n1 + 1] -= self.rho * self.reg_center
        Aeq, beq, G, h = master._split_rows(np.hstack([c.A1, np.zeros((c.A1.shape[0], 3))]), c.b1, c.sense1)
        Gc = np.zeros((len(alpha), nz))
        Gc[:, :n1 + 1] = beta
        Gc[np.arange(len(alpha)), n1 + 1 + var] = -1.0
        Gb, hb = master._bound_rows(c.sp1.ylb, c.sp1.yub, nz)
        Gt = np.zeros((1, nz))
        Gt[0, n1 + 2] = -1.0              # tau >= 0
        res = master.qp_solve(H, g, Aeq, beq, np.vstack([G, Gc, Gb, Gt]), np.concatenate([h, -alpha, hb, [0.0]]))
        lam = res.lam[G.shape[0]:G.shape[0] + len(alpha)]
        const = 0.5 * self.rho * float(self.reg_center @ self.reg_center) if self.reg_center is not None else 0.0
        return res, lam, res.obj + const

    def remove_cuts_by_multiplier(self, tol=cut_pool.CUT_REMOVE_TOLERANCE):
        """algorithm.jl:57-72 on both row sets: a mean cut or a tail cut whose master row has a
        multiplier below tol leaves; the incumbent rows never do."""
        epi = self.cell.epi[0]
        if self._mean_duals is None:
            return
        epi.cuts[:] = [cut for j, cut in enumerate(epi.cuts) if j >= len(self._mean_duals) or abs(self._mean_duals[j]) >= tol]
        self.tail_cuts[:] = [cut for j, cut in enumerate(self.tail_cuts)
                             if j >= len(self._tail_duals) or abs(self._tail_duals[j]) >= tol]


def sd_iteration(cell: RiskCell, scenario_list, update_incumbent_cut=True, quad_scalar_schedule=None, tie_rel=0.0,
                 feasibility=False, keep_picks=False):
    """One SD iteration on the mean-CVaR master: master.sd_iteration's steps with the tail cut taken
    right after each mean cut (twosd.cut_tail at the eta of the cut's point) and (x, eta) as the
    master point.  keep_picks: every new mean cut keeps its pick handle and every new tail row its
    tail handle (for bootstrap_gap_test), and the handles of rows that left are released: the live
    handles are then len(epi.cuts) + len(cell.tail_cuts) + 2.  lam == 0: master.sd_iteration on the
    wrapped cell itself."""
    if feasibility:
        raise ValueError("risk.sd_iteration: feasibility rows are not supported for the composite objective")
    if cell.risk.lam == 0.0:
        master.sd_iteration(cell.cell, scenario_list, update_incumbent_cut=update_incumbent_cut,
                            quad_scalar_schedule=quad_scalar_schedule, tie_rel=tie_rel, keep_picks=keep_picks)
        cell.improvement_info = cell.cell.improvement_info
        return
    if quad_scalar_schedule is None:
        quad_scalar_schedule = master.ConstantQuadScalarSchedule(0.1)
    c = cell.cell
    assert len(scenario_list) == len(c.epi) == 1
    epi, V = c.epi[0], c.dual_vertices
    vals = [np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in scenario_list]
    twosd.sd_iteration_solve(c.epi, vals, c.x_candidate, c.x_incumbent, V)
    if cell.master_status == master.OPTIMAL:
        cell.remove_cuts_by_multiplier()
    info_last = cell.composite()
    cut = twosd.build_sasa_cut(epi, c.x_candidate, V, tie_rel, keep_picks=keep_picks)
    if cell.eta_candidate is None:      # the first iteration: eta starts at the sample's VaR at the candidate
        cell.eta_candidate = cell.eta_incumbent = twosd.cut_quantile(epi, cell.risk.level).var
    epi.cuts.append(cut)
    cell.tail_cuts.append(tail_row(twosd.cut_tail(epi, cell.eta_candidate, keep=keep_picks), cut.weight_mark))
    if update_incumbent_cut:
        epi.incumbent_cut = twosd.build_sasa_cut(epi, c.x_incumbent, V, tie_rel, keep_picks=keep_picks)
        cell.tail_incumbent = tail_row(twosd.cut_tail(epi, cell.eta_incumbent, keep=keep_picks), epi.incumbent_cut.weight_mark)
    if keep_picks:   # removed rows and the replaced incumbent rows no longer need their handles
        live = [r.picks for r in cell.tail_cuts + [cell.tail_incumbent] if r is not None and r.picks is not None]
        twosd.release_unused_picks(epi, keep=live)
    zc = np.append(c.x_candidate, cell.eta_candidate)
    zi = np.append(c.x_incumbent, cell.eta_incumbent)
    cell.improvement_info = c.improvement_info = twosd.check_improvement(
        info_last, cell.composite(), cell.objf_original(c.x_candidate, cell.eta_candidate),
        cell.objf_original(c.x_incumbent, cell.eta_incumbent), zc, zi)
    rho = quad_scalar_schedule(cell)
    if cell.improvement_info.is_improved:
        c.x_incumbent = c.x_candidate.copy()
        cell.eta_incumbent = cell.eta_candidate
    cell.add_regularization(c.x_incumbent, cell.eta_incumbent, rho)
    c.x_candidate, cell.eta_candidate = cell.solve_master()


def sd_run(cell: RiskCell, next_scenarios, max_iter, **iteration_args):
    """max_iter iterations of sd_iteration(cell, next_scenarios(it)): a fixed count, returned as an
    int.  The loop with the stopping rule is sd_run_stop: no stop= argument here, and
    feasibility=True raises ValueError."""
    if "stop" in iteration_args:
        raise TypeError("risk.sd_run takes no stop= (a fixed number of iterations; the loop with the stopping rule "
                        "is risk.sd_run_stop)")
    if iteration_args.get("feasibility"):
        raise ValueError("risk.sd_run: feasibility rows are not supported for the composite objective")
    for it in range(int(max_iter)):
        sd_iteration(cell, next_scenarios(it), **iteration_args)
    return int(max_iter)


def _rows_with_picks(cell: RiskCell):
    """(mean cuts, has incumbent, tail rows, has incumbent tail) of the cell, every one with its handle."""
    epi = cell.cell.epi[0]
    mean = stopping._epigraph_cuts(epi, 0)
    tails = list(cell.tail_cuts) + ([cell.tail_incumbent] if cell.tail_incumbent is not None else [])
    for j, row in enumerate(tails):
        if row.picks is None:
            which = "incumbent tail row" if (cell.tail_incumbent is not None and j == len(tails) - 1) else f"tail row {j}"
            raise ValueError(f"bootstrap_gap_test: {which} carries no picks; run the iterations with keep_picks=True "
                             "(risk.sd_iteration / risk.sd_run_stop)")
    return mean, epi.incumbent_cut is not None, tails, cell.tail_incumbent is not None


def bootstrap_gap_test(cell: RiskCell, M=32, seed=0, eps=1e-3, frac=0.95, index_offset=0, reform=None,
                       sampling=None) -> "stopping.GapTest":
    """stopping.bootstrap_gap_test for the composite objective, at the incumbent (x^, eta^).

    One reform_cuts call re-forms the mean cuts, the incumbent cut, the tail rows' tail handles and the
    incumbent tail's under the identity weights (b = 0) and M Poisson(1) replicates.  With
    total_b = total_weight[b], the rows of replicate b in master_rows() order:
        mean rows      those of stopping.bootstrap_gap_test, on variable 0
        tail rows      tau >= (W_t,jb / total_b) (alpha_jb + beta_jb'x - eta)
        incumbent tail tau >= (W_t,b / W_inc,b) (...), W_inc,b the re-formed incumbent mean cut's
                       weight_mark; dropped when that is 0
        tau >= 0       always (solve_master_rows)
    U_b = c'x^ + lam eta^ + w_mean max(mean rows at x^, lower bound) + w_tail max(tail rows at (x^, eta^), 0),
    L_b = solve_master_rows over those rows; gaps, threshold, fraction and passed as in the
    risk-neutral test.  rows0: replicate 0's (var, alpha, beta); rows: every replicate's.
    The tail sets are fixed at each row's own (x, eta) and the resampling is a Poisson(1) bootstrap:
    DESIGN.md §9.  lam == 0: stopping.bootstrap_gap_test on the wrapped cell.
    reform(epi, cuts, M, seed, index_offset) replaces twosd.reform_cuts (tests): its cuts are sdCut
    objects, a tail row's the tail cut behind it with weight_mark = the tail's weight."""
    if cell.risk.lam == 0.0:
        return stopping.bootstrap_gap_test(cell.cell, M=M, seed=seed, eps=eps, frac=frac, index_offsets=[index_offset],
                                           reform=reform, sampling=sampling)
    if M < 1:
        raise ValueError("bootstrap_gap_test: M must be at least 1")
    reform = twosd.reform_cuts if reform is None else reform
    c = cell.cell
    epi = c.epi[0]
    n1 = c.n1
    mean, has_inc, tails, has_tinc = _rows_with_picks(cell)
    nc, nt = len(epi.cuts), len(cell.tail_cuts)
    kw = {} if sampling is None else {"sampling": sampling}
    R = reform(epi, mean + [_tail_of_row(r) for r in tails], M, seed, index_offset, **kw)
    o_t = len(mean)                                    # the first tail handle's column
    z = np.append(np.asarray(c.x_incumbent, dtype=np.float64), float(cell.eta_incumbent))
    cz = cell.objf_original(z[:n1], z[n1])
    wm, wt = cell.weights()
    lb = epi.lower_bound
    U, L, rows = np.zeros(M + 1), np.zeros(M + 1), []

    def over_z(a, beta_x, d, eta_coef):
        return d * a, np.append(d * np.asarray(beta_x, dtype=np.float64), eta_coef)
    for b in range(M + 1):
        tw = float(R.total_weight[b])
        var, ra, rb = [], [], []
        # the mean rows: stopping.bootstrap_gap_test's (a replicate that drew nothing leaves the lower bound)
        if tw > 0.0:
            for j in range(nc):
                d = float(R.weight_mark[b, j]) / tw
                a, be = over_z(R.alpha[b, j], R.beta[b, j], d, 0.0)
                var.append(0); ra.append(a + (1 - d) * lb); rb.append(be)
        w_inc = float(R.weight_mark[b, nc]) if has_inc else 0.0
        if has_inc:
            if w_inc == 0.0:
                var.append(0); ra.append(lb); rb.append(np.zeros(n1 + 1))
            else:
                var.append(0); ra.append(float(R.alpha[b, nc])); rb.append(np.append(R.beta[b, nc], 0.0))
        if not var:
            var.append(0); ra.append(lb); rb.append(np.zeros(n1 + 1))
        n_mean = len(var)
        # the tail rows: tau >= d (alpha + beta'x - eta), d the tail's share of the replicate's weight
        if tw > 0.0:
            for j in range(nt):
                d = float(R.weight_mark[b, o_t + j]) / tw
                a, be = over_z(R.alpha[b, o_t + j], R.beta[b, o_t + j], d, -d)
                var.append(1); ra.append(a); rb.append(be)
        if has_tinc and w_inc > 0.0:
            d = float(R.weight_mark[b, o_t + nt]) / w_inc
            a, be = over_z(R.alpha[b, o_t + nt], R.beta[b, o_t + nt], d, -d)
            var.append(1); ra.append(a); rb.append(be)
        var, ra, rb = np.array(var, dtype=np.int64), np.array(ra), np.array(rb).reshape(len(ra), n1 + 1)
        at_z = ra + rb @ z
        m_val = max(lb, float(at_z[:n_mean].max()))
        t_val = max(0.0, float(at_z[n_mean:].max())) if len(ra) > n_mean else 0.0
        res, _, obj = cell.solve_master_rows(var, ra, rb)
        if res.status != master.OPTIMAL:
            raise RuntimeError(f"bootstrap_gap_test: master of replicate {b} not solved: {res.status}")
        U[b], L[b] = cz + wm * m_val + wt * t_val, obj
        rows.append((var, ra, rb))
    gaps = U - L
    thr = eps * (1.0 + abs(U[0]))
    fraction = float(np.count_nonzero(gaps[1:] <= thr)) / M
    return stopping.GapTest(U, L, gaps, thr, fraction, fraction >= frac, rows[0], tuple(rows))


def sd_run_stop(cell: RiskCell, next_scenarios, max_iter, min_iter=0, check_every=10, stop=None, sampling=None,
                stop_args=None, **iteration_args):
    """master.sd_run for the composite objective: sd_iteration(cell, next_scenarios(it), keep_picks=True)
    for it = 0, 1, ... and, every check_every iterations once min_iter have run, stop(cell) --
    default bootstrap_gap_test(cell, sampling=sampling, **stop_args) -- ending when its result has
    .passed, or after max_iter.  Returns (iterations run, the last test result or None)."""
    if check_every < 1:
        raise ValueError("check_every must be at least 1")
    if iteration_args.get("feasibility"):
        raise ValueError("risk.sd_run_stop: feasibility rows are not supported for the composite objective")
    if stop is None:
        def stop(c):
            return bootstrap_gap_test(c, sampling=sampling, **(stop_args or {}))
    result = None
    it = 0
    while it < max_iter:
        sd_iteration(cell, next_scenarios(it), keep_picks=True, **iteration_args)
        it += 1
        if it >= min_iter and it % check_every == 0:
            result = stop(cell)
            if result.passed:
                break
    return it, result
