"""Shared cases of the general-bounds tests (tests/test_host_bounds.py, tests/test_gpu_bounds.py):
the instances, a numpy restatement of the canonical-form table (the tests' own, independent of
the library's), and HiGHS solves of the bounded LPs (oracle.lp_highs.solve_rhs)."""
from __future__ import annotations

import dataclasses
import functools
from types import SimpleNamespace

import numpy as np

from oracle import lp_highs
from sqlp_amd import smps

INF = np.inf


def dense_to_csc(W):
    W = np.asarray(W, dtype=np.float64)
    cp, rv, nz = [0], [], []
    for j in range(W.shape[1]):
        i = np.nonzero(W[:, j])[0]
        rv += i.tolist()
        nz += W[i, j].tolist()
        cp.append(len(rv))
    return np.array(cp, dtype=np.int64), np.array(rv, dtype=np.int64), np.array(nz, dtype=np.float64)


def stage_problem(W, T, q, r, sense, lb, ub):
    """Product-side spStageProblem of a dense template."""
    m, n2 = W.shape
    return smps.spStageProblem(
        last_stage_vars=[f"x{j}" for j in range(T.shape[1])], current_stage_vars=[f"y{j}" for j in range(n2)],
        stage_constraints=[f"r{i}" for i in range(m)], sense=list(sense), q=np.asarray(q, dtype=np.float64),
        r=np.asarray(r, dtype=np.float64), T=dense_to_csc(T), W=dense_to_csc(W),
        ylb=np.asarray(lb, dtype=np.float64), yub=np.asarray(ub, dtype=np.float64))


def highs_problem(W, q, sense, lb, ub):
    """What oracle.lp_highs.solve_rhs reads: the bounded LP itself."""
    return SimpleNamespace(W=np.asarray(W, dtype=np.float64), q=np.asarray(q, dtype=np.float64), senses=list(sense),
                           cur_lb=np.asarray(lb, dtype=np.float64), cur_ub=np.asarray(ub, dtype=np.float64))


def highs_objectives(hp, B):
    """HiGHS objective of the bounded LP for every rhs row of B (all must be optimal)."""
    out = np.zeros(len(B))
    for s, b in enumerate(B):
        st, obj, _, _ = lp_highs.solve_rhs(hp, b)
        assert st == 0, f"rhs {s}: HiGHS status {st}"
        out[s] = obj
    return out


def canon_np(W, q, r, sense, lb, ub):
    """The table of the canonical form, restated in numpy on dense arrays.  Returns a namespace:
    W (m_lp x n_lp), q, r, sense, c0, nb, and back(y') -> y."""
    W = np.asarray(W, dtype=np.float64)
    m2, n2 = W.shape
    s = np.zeros(n2)
    cols, costs, back = [], [], []          # back[j] = (offset, sign, lp column or None, second column or None)
    boxed, free = [], []
    for j in range(n2):
        lo, hi = lb[j], ub[j]
        assert lo <= hi and lo < INF and hi > -INF
        if np.isfinite(lo) and hi == INF:                 # default / LO
            s[j] = lo
            back.append([lo, 1.0, len(cols), None]); cols.append(W[:, j]); costs.append(q[j])
        elif lo == -INF and np.isfinite(hi):              # MI + UP: negated
            s[j] = hi
            back.append([hi, -1.0, len(cols), None]); cols.append(-W[:, j]); costs.append(-q[j])
        elif lo == -INF and hi == INF:                    # FR
            back.append([0.0, 1.0, len(cols), None]); cols.append(W[:, j]); costs.append(q[j]); free.append(j)
        elif lo == hi:                                    # FX: eliminated
            s[j] = lo
            back.append([lo, 1.0, None, None])
        else:                                             # boxed
            s[j] = lo
            back.append([lo, 1.0, len(cols), None]); cols.append(W[:, j]); costs.append(q[j]); boxed.append(j)
    for j in free:
        back[j][3] = len(cols); cols.append(-W[:, j]); costs.append(-q[j])
    nb = len(boxed)
    Wc = np.zeros((m2 + nb, len(cols)))
    Wc[:m2] = np.array(cols).T
    rc = np.concatenate([np.asarray(r, dtype=np.float64) - W @ s, np.zeros(nb)])
    for b, j in enumerate(boxed):
        Wc[m2 + b, back[j][2]] = 1.0
        rc[m2 + b] = ub[j] - lb[j]

    def map_back(yp):
        yp = np.atleast_2d(yp)
        y = np.zeros((yp.shape[0], n2))
        for j, (off, sg, a, b2) in enumerate(back):
            y[:, j] = off
            if a is not None:
                y[:, j] += sg * yp[:, a]
            if b2 is not None:
                y[:, j] -= yp[:, b2]
        return y

    return SimpleNamespace(W=Wc, q=np.array(costs), r=rc, sense=list(sense) + ["L"] * nb, c0=float(np.dot(q, s)), nb=nb,
                           s=s, boxed=boxed, back=map_back)


# ---- the toy: 3 rows x 6 columns, one column of every kind --------------------------------------
TOY_W = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
                  [1.0, -1.0, 0.0, 2.0, 0.0, 1.0],
                  [0.0, 1.0, 1.0, -1.0, 1.0, 0.0]])
TOY_SENSE = ["G", "L", "E"]
TOY_Q = np.array([3.0, 2.0, -1.0, 0.5, 4.0, 1.0])
TOY_R = np.array([4.0, 6.0, 1.0])
#            default  LO     MI+UP  FR     FX    boxed
TOY_LB = np.array([0.0, 0.5, -INF, -INF, 1.5, 0.25])
TOY_UB = np.array([INF, INF, 2.0, INF, 1.5, 1.0])
TOY_T = np.array([[1.0, 0.0], [0.0, 0.5], [0.25, 0.0]])
TOY_X = np.array([0.5, 1.0])
TOY_ROWS = np.array([0, 1, 2])       # every rhs entry is random


def toy_values(N=16, seed=11):
    """N scenario rhs vectors (the caller's space) around TOY_R."""
    return TOY_R + np.random.default_rng(seed).uniform(-1.5, 1.5, size=(N, 3))


# ---- lands with bounds ---------------------------------------------------------------------------
def lands_bounds(n2):
    lb, ub = np.zeros(n2), np.full(n2, INF)
    ub[0], ub[4], ub[8] = 1.5, 2.0, 2.0
    lb[11] = 0.25
    lb[5], ub[5] = 0.5, 1.0
    return lb, ub


@functools.lru_cache(maxsize=None)
def lands():
    """(instance dict, bounded product sp2, bounded oracle sp2, HiGHS problem)."""
    from tests import instances as I
    inst = I.load("lands")
    lb, ub = lands_bounds(len(inst["sp2"].q))
    sp2 = dataclasses.replace(inst["sp2"], ylb=lb, yub=ub)
    osp2 = dataclasses.replace(inst["osp2"], cur_lb=lb.copy(), cur_ub=ub.copy())
    return inst, sp2, osp2, highs_problem(osp2.W, osp2.q, osp2.senses, lb, ub)


def lands_xs():
    from tests import instances as I
    xe = I.x_ev("lands")
    return [xe, 1.2 * xe, np.array([3.0, 3.0, 3.0, 3.0]), np.array([2.0, 4.0, 3.0, 4.0])]


def lands_rhs(osp2, rows, x, values):
    """b = r_w - T x of every scenario (values: N x k in the caller's space, RHS elements)."""
    B = np.tile(osp2.r - osp2.T @ x, (len(values), 1))
    B[:, rows] += values - osp2.r[rows]
    return B


@functools.lru_cache(maxsize=None)
def lands_highs_by_demand(xi):
    """HiGHS objective of bounded lands at lands_xs()[xi] for every support value of the random
    element(s): {values tuple: objective} (lands has one element with three values)."""
    inst, sp2, osp2, hp = lands()
    pos, rows, cols = smps.scenario_positions(sp2, inst["sto"])
    assert len(pos) == 1 and cols[0] < 0
    support = inst["sto"].indep[pos[0]][1]
    x = lands_xs()[xi]
    vals = np.array(support, dtype=np.float64)[:, None]
    objs = highs_objectives(hp, lands_rhs(osp2, rows, x, vals))
    return {float(v): float(o) for v, o in zip(support, objs)}


def lands_highs(xi, values):
    table = lands_highs_by_demand(xi)
    return np.array([table[float(v[0])] for v in values])


# ---- synthetic complete-recourse template crossing the 64-row slot -------------------------------
@functools.lru_cache(maxsize=None)
def slot_template(m2=60, nA=40, n1=4, nboxed=10, seed=5):
    """W = [A | I | -I], all rows 'E', penalty columns at cost 50: every rhs is feasible.  Columns
    0..nboxed-1 of A are boxed, column nboxed is free, column nboxed + 1 is (-inf, hi].  The costs
    are q_j = A_j . pi0 + slack for a fixed |pi0| <= 1 (slack 0 for the free column, < 0 for the
    negated one), so pi0 is dual feasible and every LP is bounded."""
    rng = np.random.default_rng(seed)
    A = np.zeros((m2, nA))
    for j in range(nA):
        i = rng.choice(m2, size=4, replace=False)
        A[i, j] = rng.uniform(0.5, 2.0, size=4) * rng.choice([-1.0, 1.0], size=4)
    W = np.hstack([A, np.eye(m2), -np.eye(m2)])
    pi0 = rng.uniform(-1.0, 1.0, size=m2)
    qA = A.T @ pi0 + rng.uniform(0.5, 2.0, size=nA)
    jf, jn = nboxed, nboxed + 1
    qA[jf] = A[:, jf] @ pi0
    qA[jn] = A[:, jn] @ pi0 - 0.5
    q = np.concatenate([qA, np.full(2 * m2, 50.0)])
    n2 = W.shape[1]
    lb, ub = np.zeros(n2), np.full(n2, INF)
    lb[:nboxed] = rng.uniform(0.0, 0.5, size=nboxed)
    ub[:nboxed] = lb[:nboxed] + rng.uniform(0.5, 1.5, size=nboxed)
    lb[jf] = -INF
    lb[jn], ub[jn] = -INF, 1.0
    T = np.zeros((m2, n1))
    for j in range(n1):
        i = rng.choice(m2, size=6, replace=False)
        T[i, j] = rng.uniform(-1.0, 1.0, size=6)
    r = rng.uniform(-2.0, 2.0, size=m2)
    rows = np.sort(rng.choice(m2, size=8, replace=False)).astype(np.int32)
    sense = ["E"] * m2
    return SimpleNamespace(W=W, T=T, q=q, r=r, sense=sense, lb=lb, ub=ub, rows=rows,
                           sp2=stage_problem(W, T, q, r, sense, lb, ub))


def highs_objectives_blocked(W, q, sense, lb, ub, B, block=64):
    """HiGHS objectives of many rhs rows of one bounded LP: `block` scenarios per solve as one
    block-diagonal LP (the optimum of a separable LP is the blocks' optima), the objective of each
    block read from its own part of the solution.  All rows must be 'E'."""
    from scipy import sparse
    from scipy.optimize import linprog
    assert all(s == "E" for s in sense)
    m, n = W.shape
    Ws = sparse.csr_matrix(W)
    out = np.zeros(len(B))
    bounds1 = [(None if l == -INF else l, None if u == INF else u) for l, u in zip(lb, ub)]
    for a in range(0, len(B), block):
        Bs = B[a:a + block]
        nbk = len(Bs)
        res = linprog(np.tile(q, nbk), A_eq=sparse.block_diag([Ws] * nbk, format="csr"), b_eq=Bs.ravel(),
                      bounds=bounds1 * nbk, method="highs")
        assert res.status == 0, res.message
        out[a:a + nbk] = res.x.reshape(nbk, n) @ q
    return out
