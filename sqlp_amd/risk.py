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
the risk-neutral loop bit for bit.  Feasibility rows and the bootstrap stopping rule are out of
scope here (sd_run runs a fixed number of iterations).
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from . import cut_pool, master, twosd
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
    return twosd.sdCut(d * tail.alpha, np.append(d * tail.beta, -d), float(weight_mark))


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
        c = self.cell
        n1 = c.n1
        nz = n1 + 3
        var, alpha, beta = self.master_rows()
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
        self.master_status = res.status
        if res.status != master.OPTIMAL:
            raise RuntimeError(f"master not solved: {res.status}")
        lam = res.lam[G.shape[0]:G.shape[0] + len(alpha)]
        epi = c.epi[0]
        nm = len(epi.cuts)
        n_mean_rows = int(np.sum(var == 0))
        self._mean_duals = lam[:nm]
        self._tail_duals = lam[n_mean_rows:n_mean_rows + len(self.tail_cuts)]
        const = 0.5 * self.rho * float(self.reg_center @ self.reg_center) if self.reg_center is not None else 0.0
        self.master_obj = res.obj + const
        return res.z[:n1].copy(), float(res.z[n1])

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
                 feasibility=False):
    """One SD iteration on the mean-CVaR master: master.sd_iteration's steps with the tail cut taken
    right after each mean cut (twosd.cut_tail at the eta of the cut's point) and (x, eta) as the
    master point.  lam == 0: master.sd_iteration on the wrapped cell itself."""
    if feasibility:
        raise ValueError("risk.sd_iteration: feasibility rows are not supported for the composite objective")
    if cell.risk.lam == 0.0:
        master.sd_iteration(cell.cell, scenario_list, update_incumbent_cut=update_incumbent_cut,
                            quad_scalar_schedule=quad_scalar_schedule, tie_rel=tie_rel)
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
    cut = twosd.build_sasa_cut(epi, c.x_candidate, V, tie_rel)
    if cell.eta_candidate is None:      # the first iteration: eta starts at the sample's VaR at the candidate
        cell.eta_candidate = cell.eta_incumbent = twosd.cut_quantile(epi, cell.risk.level).var
    epi.cuts.append(cut)
    cell.tail_cuts.append(tail_row(twosd.cut_tail(epi, cell.eta_candidate), cut.weight_mark))
    if update_incumbent_cut:
        epi.incumbent_cut = twosd.build_sasa_cut(epi, c.x_incumbent, V, tie_rel)
        cell.tail_incumbent = tail_row(twosd.cut_tail(epi, cell.eta_incumbent), epi.incumbent_cut.weight_mark)
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
    """max_iter iterations of sd_iteration(cell, next_scenarios(it)).  There is no stopping rule for
    the composite objective: no stop= argument, and feasibility=True raises ValueError."""
    if "stop" in iteration_args:
        raise TypeError("risk.sd_run takes no stop= (no stopping rule for the composite objective)")
    if iteration_args.get("feasibility"):
        raise ValueError("risk.sd_run: feasibility rows are not supported for the composite objective")
    for it in range(int(max_iter)):
        sd_iteration(cell, next_scenarios(it), **iteration_args)
    return int(max_iter)
