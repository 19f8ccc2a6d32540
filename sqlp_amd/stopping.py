"""In-sample stopping rule of SD: the bootstrap of the gap at the incumbent.

The reference has no stopping rule (its readme lists "Need to implement stopping criteria";
src/sd_algorithm/plugin/stopping_rule.jl is an empty file): its drivers run a fixed number of
iterations.  The rule here is SD's own (Higle and Sen; Sen and Liu 2016): resample the
observations, re-form every cut the master holds from the argmax picks it was built with
(twosd.reform_cuts: no argmax is repeated, a cut is linear in the scenario weights), and compare
the re-formed upper estimate at the incumbent with the value of the re-formed master.  Stop when
nearly all replicates show a small gap.

The resampling is a Poisson(1) bootstrap (independent counts per observation and replicate, every
sum normalised by the replicate's own total weight), not the multinomial resample of the
literature: DESIGN.md §9.  The observations of an i.i.d. epigraph are its scenarios; those of an
epigraph filled from a variance-reduced stream (twosd.Sampling) are its groups, and `sampling=`
makes the bootstrap resample whole groups.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import twosd


@dataclass
class GapTest:
    """bootstrap_gap_test's result.  Index 0 is the identity replicate (the cell's own cuts),
    1..M the bootstrap replicates."""
    U: np.ndarray          # c'x^ + sum_e w_e max(re-formed cuts of e at x^), floored by the lower bound
    L: np.ndarray          # value of the regularised master over the re-formed rows
    gaps: np.ndarray       # U - L
    threshold: float       # eps (1 + |U_0|)
    fraction: float        # share of the replicates 1..M with gap <= threshold
    passed: bool           # fraction >= frac
    rows0: tuple = ()      # (epi, alpha, beta) master rows of the identity replicate, in sync_cuts' order
    rows: tuple = ()       # every replicate's (variable, alpha, beta) rows (risk.bootstrap_gap_test fills it)


def _epigraph_cuts(epi, e):
    cuts = list(epi.cuts) + ([epi.incumbent_cut] if epi.incumbent_cut is not None else [])
    if not cuts:
        raise ValueError(f"bootstrap_gap_test: epigraph {e} holds no cut")
    for j, cut in enumerate(cuts):
        if cut.picks is None:
            which = "incumbent cut" if (epi.incumbent_cut is not None and j == len(cuts) - 1) else f"cut {j}"
            raise ValueError(f"bootstrap_gap_test: {which} of epigraph {e} carries no picks; run the iterations with "
                             "keep_picks=True (master.sd_iteration / master.sd_run)")
    return cuts


def _plans(sampling, E):
    """One plan (or None) per epigraph from bootstrap_gap_test's sampling= argument."""
    if sampling is None or isinstance(sampling, twosd.Sampling):
        return [sampling] * E
    plans = list(sampling)
    if len(plans) != E:
        raise ValueError(f"bootstrap_gap_test: sampling lists {len(plans)} plans for {E} epigraphs")
    return plans


def bootstrap_gap_test(cell, M=32, seed=0, eps=1e-3, frac=0.95, index_offsets=None, reform=None, sampling=None) -> GapTest:
    """The bootstrap gap test at the cell's incumbent x^ = cell.x_incumbent.

    Every cut of every epigraph of the cell (epi.cuts and the incumbent cut) must carry picks.
    For b = 0..M with replicate b's re-formed cuts (b = 0: the identity weights):
        U_b = c'x^ + sum_e w_e evaluate_epigraph(cuts_b, incumbent_b, x^, total_weight_b, lower bound)
              (discount weight_mark_jb / total_weight_b; the incumbent cut discount 1, as sync_cuts)
        L_b = value of the cell's regularised master (its rho and centre) over those rows (qp_solve)
        gap_b = U_b - L_b
    fraction = #{b >= 1 : gap_b <= eps (1 + |U_0|)} / M and passed = fraction >= frac.  eps and
    frac are parameters (defaults: the prox schedule's tolerance 1e-3, and 0.95), not acceptance
    thresholds of the library.  Epigraph e draws its counts from the stream seed + e, its first
    scenario at global index index_offsets[e] (default 0).  sampling: the twosd.Sampling plan the
    epigraphs were filled with, or a list with one plan (or None) per epigraph: the replicates of
    such an epigraph resample whole groups (reform is then called with the keyword sampling=).
    reform(epi, cuts, M, seed, index_offset) replaces twosd.reform_cuts (tests)."""
    if M < 1:
        raise ValueError("bootstrap_gap_test: M must be at least 1")
    reform = twosd.reform_cuts if reform is None else reform
    x = np.asarray(cell.x_incumbent, dtype=np.float64)
    E = len(cell.epi)
    offs = [0] * E if index_offsets is None else list(index_offsets)
    plans = _plans(sampling, E)
    per_epi = []
    for e, epi in enumerate(cell.epi):
        cuts = _epigraph_cuts(epi, e)
        kw = {} if plans[e] is None else {"sampling": plans[e]}
        per_epi.append((epi, len(epi.cuts), epi.incumbent_cut is not None, reform(epi, cuts, M, seed + e, offs[e], **kw)))
    cx = cell.objf_original(x)
    U = np.zeros(M + 1)
    L = np.zeros(M + 1)
    for b in range(M + 1):
        u = cx
        rows_e, rows_a, rows_b = [], [], []
        for e, (epi, nc, has_inc, R) in enumerate(per_epi):
            tw = float(R.total_weight[b])
            lb = epi.lower_bound
            # a replicate that drew no scenario at all leaves only the lower bound (discount 0)
            cuts_b = [R.cut(b, j) for j in range(nc)] if tw > 0.0 else []
            inc_b = R.cut(b, nc) if has_inc else None
            if inc_b is not None and inc_b.weight_mark == 0.0:   # no scenario drawn: the lower bound, not the zero cut
                inc_b = twosd.sdCut(lb, np.zeros(cell.n1), 0.0)
            u += epi.objective_weight * twosd.evaluate_epigraph(cuts_b, inc_b, x, tw if tw > 0.0 else 1.0, lb)
            for cut in cuts_b:                      # add_cut_to_master (epigraph.jl:101-117)
                d = cut.weight_mark / tw
                rows_e.append(e); rows_a.append(d * cut.alpha + (1 - d) * lb); rows_b.append(d * cut.beta)
            if inc_b is not None:
                rows_e.append(e); rows_a.append(inc_b.alpha); rows_b.append(np.asarray(inc_b.beta, dtype=np.float64))
            if not cuts_b and inc_b is None:        # keep the master bounded: eta_e >= lower bound
                rows_e.append(e); rows_a.append(lb); rows_b.append(np.zeros(cell.n1))
        res, _, obj = cell.solve_master_rows(np.array(rows_e), np.array(rows_a), np.array(rows_b).reshape(len(rows_a), cell.n1))
        if res.status != "OPTIMAL":
            raise RuntimeError(f"bootstrap_gap_test: master of replicate {b} not solved: {res.status}")
        U[b], L[b] = u, obj
        if b == 0:
            rows0 = (np.array(rows_e), np.array(rows_a), np.array(rows_b).reshape(len(rows_a), cell.n1))
    gaps = U - L
    thr = eps * (1.0 + abs(U[0]))
    fraction = float(np.count_nonzero(gaps[1:] <= thr)) / M
    return GapTest(U, L, gaps, thr, fraction, fraction >= frac, rows0)
