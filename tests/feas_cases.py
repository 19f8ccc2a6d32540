"""Case builders of the feasibility-ray tests (tests/test_gpu_feas_rays.py, test_gpu_feas_scan.py,
test_gpu_feas_loop.py, test_feas_host.py): instances WITHOUT relatively complete recourse.

* lands3f: lands' own core and time files with a six-point joint distribution of the three demand
  rows; two of the points have a total demand (13, 14) above the capacity lands' x_EV installs (12),
  and lands has no unmet-demand slack, so their stage-2 LPs are infeasible there.
* incomplete(...): a generated transport-like template: L capacity rows fed by x through T, G demand
  rows, one E row, no slack column; optionally boxed arcs (bound rows, mv > m2).  Random elements are
  demand right-hand sides and T entries of capacity rows.

A plain helper module, like tests/synth_cases.py."""
from __future__ import annotations

import functools
import os
from types import SimpleNamespace

import numpy as np

from tests import bounds_cases as BC
from tests import instances as I

# ---- lands3f ---------------------------------------------------------------------------------------
LANDS3F_ROWS = ("S2C5", "S2C6", "S2C7")
LANDS3F_POINTS = np.array([[3.0, 3.0, 2.0], [5.0, 3.0, 2.0], [7.0, 3.0, 2.0], [5.0, 2.0, 3.0], [7.0, 4.0, 2.0], [7.0, 4.0, 3.0]])
LANDS3F_PROBS = np.array([0.15, 0.25, 0.15, 0.20, 0.15, 0.10])
LANDS3F_RECOURSE = [174.4, 258.6667, 360.6667, 236.1667]      # HiGHS at x_EV, the four feasible points
LANDS3F_INFEASIBLE = [4, 5]
LANDS3F_OPT = 423.216667                                       # extensive form over the six points
LANDS3F_MIN_CAPACITY = 14.0                                    # every feasible x has sum(x) >= 14


@functools.lru_cache(maxsize=None)
def lands3f():
    """lands' cor / tim (data/smps/lands) with the six-point block built in code.  Returns a
    namespace: sp1, sp2 (product side), osp1, osp2 (oracle side), sto, x_ev, support (6 x 3, in the
    order of the context's positions), probs."""
    from sqlp_amd import smps
    from sqlp_amd.smps import spSmpsPosition, spStoBlock, spStoType
    inst = I.load("lands")
    pos = [spSmpsPosition("RHS", r) for r in LANDS3F_ROWS]
    sto = spStoType("LandS3f")
    sto.blocks = [spStoBlock("BLOCK1", "PERIOD2", pos, LANDS3F_PROBS.tolist(), LANDS3F_POINTS.tolist())]
    sp1 = smps.get_smps_stage_template(inst["cor"], inst["tim"], 1)
    return SimpleNamespace(sp1=sp1, sp2=inst["sp2"], osp1=inst["osp1"], osp2=inst["osp2"], sto=sto, positions=pos,
                           x_ev=I.x_ev("lands"), support=LANDS3F_POINTS.copy(), probs=LANDS3F_PROBS.copy())


def lands3f_rhs(L, x, values):
    """b = r_w - T x of every scenario (values: N x 3, the three demand rows)."""
    sp = L.osp2
    rows = [sp.row_names.index(r) for r in LANDS3F_ROWS]
    B = np.tile(sp.r - sp.T @ np.asarray(x), (len(values), 1))
    B[:, rows] = values
    return B


# ---- generated incomplete-recourse template ------------------------------------------------------
N1 = 4
X0 = np.array([0.6, 0.5, 0.7, 0.55])
T_AMP = 0.3
# id: (m_lp, k, boxed, seed, demand amplitude).  The amplitude was picked from a short ladder on the
# CPU (HiGHS alone) as a value at which between a tenth and a half of the scenarios are infeasible
# at X0.
CASES = {
    "m5": (5, 3, False, 1, 1.0), "m5b": (5, 3, True, 2, 0.3),
    "m63": (63, 3, False, 3, 5.0), "m63b": (63, 3, True, 4, 4.0),
    "m64": (64, 3, False, 5, 4.0), "m64b": (64, 3, True, 6, 4.0),
    "m65": (65, 3, False, 7, 5.0), "m65b": (65, 3, True, 8, 5.0),
    "m130": (130, 3, False, 9, 4.0), "m130b": (130, 3, True, 10, 4.0),
    "m130k70": (130, 70, False, 11, 2.5), "m130bk70": (130, 70, True, 12, 2.0),
}
N_SCEN = 200


@functools.lru_cache(maxsize=None)
def incomplete(cid):
    m_lp, k, boxed, seed, amp = CASES[cid]
    return incomplete_template(m_lp, k, boxed, seed, amp, cid)


def incomplete_template(m_lp, k, boxed, seed, amp, cid="?"):
    """Rows: ns capacity rows (L): sum of the arcs out of supplier i <= r_i + u_i x[i % 4]
    (T[i, i % 4] = -u_i); nd demand rows (G): sum of the arcs into demand j >= d_j; one E row:
    sum of all arcs - z = 0.  Columns: three arcs per demand (fewer when suppliers repeat) at costs
    in (1, 3), and z at 0.1.  Nothing absorbs unmet demand.  boxed: the first nb arcs have an upper
    bound (one bound row each).  Elements: about two thirds demand right-hand sides, the rest T
    entries of capacity rows (listed by descending row, so the restated order is not the listing)."""
    rng = np.random.default_rng(7000 + seed)
    nb = (1 if m_lp <= 5 else 4) if boxed else 0
    m2 = m_lp - nb
    nd = m2 // 2
    ns = m2 - 1 - nd
    assert ns >= 1 and nd >= 1
    arcs = []
    for j in range(nd):
        for i in dict.fromkeys([j % ns, (j + 1) % ns, (3 * j + 2) % ns]):
            arcs.append((i, j))
    n2 = len(arcs) + 1
    W = np.zeros((m2, n2))
    for a, (i, j) in enumerate(arcs):
        W[i, a] = 1.0
        W[ns + j, a] = 1.0
        W[m2 - 1, a] = 1.0
    W[m2 - 1, n2 - 1] = -1.0
    q = np.concatenate([rng.uniform(1.0, 3.0, size=len(arcs)), [0.1]])
    sense = ["L"] * ns + ["G"] * nd + ["E"]
    u = rng.uniform(0.5, 1.5, size=ns)
    T = np.zeros((m2, N1))
    for i in range(ns):
        T[i, i % N1] = -u[i]
    r = np.concatenate([rng.uniform(0.5, 1.0, size=ns), rng.uniform(0.3, 0.6, size=nd), [0.0]])
    lb, ub = np.zeros(n2), np.full(n2, np.inf)
    if nb:
        ub[:nb] = rng.uniform(0.3, 0.6, size=nb)
    # elements
    nT = max(1, k // 3) if ns * 1 >= max(1, k // 3) else ns
    nR = k - nT
    assert nR <= nd and nT <= ns, (cid, k, nd, ns)
    dem = np.sort(rng.choice(nd, size=nR, replace=False))
    cap = np.sort(rng.choice(ns, size=nT, replace=False))
    elems = [(ns + int(j), -1) for j in dem] + [(int(i), int(i % N1)) for i in cap]
    elems = sorted(elems, key=lambda p: -p[0])
    rows = np.array([i for i, _ in elems], dtype=np.int32)
    cols = np.array([j for _, j in elems], dtype=np.int32)
    tmpl = np.array([r[i] if j < 0 else T[i, j] for i, j in elems])
    S = SimpleNamespace(id=cid, m_lp=m_lp, m2=m2, n2=n2, nb=nb, k=k, seed=seed, amp=amp, ns=ns, nd=nd, W=W, T=T, q=q, r=r,
                        sense=sense, lb=lb, ub=ub, elems=elems, rows=rows, cols=cols, tmpl=tmpl,
                        positions=[("RHS" if j < 0 else f"x{j}", f"r{i}") for i, j in elems],
                        sp2=BC.stage_problem(W, T, q, r, sense, lb, ub), hp=BC.highs_problem(W, q, sense, lb, ub))
    S.canon = BC.canon_np(W, q, r, sense, lb, ub)     # the LP the kernels solve: y' >= 0, bound rows appended
    return S


def values(S, N=N_SCEN, seed=1):
    """N scenario values of the k elements in listing order.  Scenario 0 is the template itself
    (feasible at X0: the basis is computed there)."""
    rng = np.random.default_rng(100 * S.seed + seed)
    uu = rng.uniform(0.0, 1.0, size=(N, S.k))
    vals = np.empty((N, S.k))
    for e, (i, j) in enumerate(S.elems):
        vals[:, e] = S.tmpl[e] + (S.amp * uu[:, e] ** 2 if j < 0 else T_AMP * (2 * uu[:, e] - 1))
    vals[0] = S.tmpl
    return vals


def coef(S, x):
    return np.array([1.0 if j < 0 else -x[j] for _, j in S.elems])


def deltas(S, x, vals):
    """DR[s][e] = coef_e(x) (value - template): what enters row rows[e] of b."""
    return (vals - S.tmpl) * coef(S, x)[None, :]


def rhs(S, x, vals):
    """b = r_w - T_w x of every scenario in the caller's space (m2 rows)."""
    B = np.tile(S.r - S.T @ x, (len(vals), 1))
    DR = deltas(S, x, vals)
    for e, i in enumerate(S.rows):
        B[:, i] += DR[:, e]
    return B


def rhs_lp(S, x, vals):
    """The right-hand sides of the canonical LP (m_lp rows: [b - W s ; hi - lo])."""
    B = rhs(S, x, vals)
    K = S.canon
    out = np.tile(K.r, (len(vals), 1))
    out[:, :S.m2] = B - (S.W @ K.s)[None, :]
    return out


def highs_status(S, x, vals):
    """HiGHS status of every scenario's bounded LP at x (0 optimal, 2 infeasible)."""
    from oracle import lp_highs
    return np.array([lp_highs.solve_rhs(S.hp, b)[0] for b in rhs(S, x, vals)])


def random_rays(S, J, seed):
    """J normalised random vectors of length m_lp with the sign pattern of a ray: >= 0 on G rows,
    <= 0 on L rows and bound rows, free on E rows; about half of the entries zero."""
    rng = np.random.default_rng(900 + seed)
    sense = list(S.canon.sense)
    F = rng.uniform(0.0, 1.0, size=(J, S.m_lp)) * (rng.uniform(size=(J, S.m_lp)) < 0.5)
    for i, s in enumerate(sense):
        if s == "L":
            F[:, i] = -F[:, i]
        elif s == "E":
            F[:, i] *= rng.choice([-1.0, 1.0], size=J)
    F[np.arange(J), rng.integers(0, S.m_lp, size=J)] = np.where(np.array(sense)[rng.integers(0, S.m_lp, size=J)] == "L", -1.0, 1.0)
    for i, s in enumerate(sense):          # the planted entries keep the pattern
        if s == "L":
            F[:, i] = -np.abs(F[:, i])
        elif s == "G":
            F[:, i] = np.abs(F[:, i])
    return F / np.abs(F).max(axis=1, keepdims=True)


# ---- the loop tests' references --------------------------------------------------------------------
def extensive_lp(c1, A1, b1, sense1, xlb, xub, W, q2, sense2, Ts, rs, probs, obj_x=None):
    """HiGHS on the extensive form over an enumerated support: x with its stage-1 rows and bounds, one
    y_s >= 0 per scenario with T_s x + W y_s (sense2) r_s.  obj_x is None: min c1'x + sum_s p_s q2'y_s;
    else max obj_x'x over the same set (the x for which every scenario's LP is feasible).  Returns
    (status, optimal value, x)."""
    from scipy.optimize import linprog
    from oracle.lp_highs import _split
    S = len(Ts)
    m1, n1 = A1.shape
    m2, n2 = W.shape
    A = np.zeros((m1 + S * m2, n1 + S * n2))
    A[:m1, :n1] = A1
    for s in range(S):
        A[m1 + s * m2:m1 + (s + 1) * m2, :n1] = Ts[s]
        A[m1 + s * m2:m1 + (s + 1) * m2, n1 + s * n2:n1 + (s + 1) * n2] = W
    b = np.concatenate([b1] + [np.asarray(r, dtype=np.float64) for r in rs])
    _, _, _, A_ub, b_ub, A_eq, b_eq = _split(list(sense1) + list(sense2) * S, A, b)
    bounds = [(None if np.isinf(l) else l, None if np.isinf(u) else u) for l, u in zip(xlb, xub)] + [(0, None)] * (S * n2)
    if obj_x is None:
        c = np.concatenate([c1] + [p * np.asarray(q2) for p in probs])
    else:
        c = np.concatenate([-np.asarray(obj_x, dtype=np.float64), np.zeros(S * n2)])
    res = linprog(c, A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=b_eq, bounds=bounds, method="highs")
    if res.status != 0:
        return res.status, np.nan, None
    return 0, float(res.fun if obj_x is None else -res.fun), res.x[:n1]


def scenario_T_r(S, v):
    """(T_w, r_w) of the scenario with element values v (listing order) of a generated template."""
    T, r = S.T.copy(), S.r.copy()
    for e, (i, j) in enumerate(S.elems):
        if j < 0:
            r[i] = v[e]
        else:
            T[i, j] = v[e]
    return T, r


# stage 1 of the generated template's loop: min c'x, sum(x) <= 40, 0 <= x <= 12
LOOP_C1 = np.array([1.0, 1.2, 0.9, 1.1])
LOOP_SUPPORT = 12


def loop_stage1():
    return BC.stage_problem(np.ones((1, N1)), np.zeros((1, 0)), LOOP_C1, np.array([40.0]), ["L"], np.zeros(N1), np.full(N1, 12.0))
