"""Generated stage-2 templates that sit exactly on the dispatch edges of the LP kernel
(lp_hyper_kernel<R, C>: R rows per lane, C column slots per lane) and of the cut's argmax kernels
(KB blocks of four k-rows), shared by tests/test_synth_cases.py (the conditions on the inputs,
proved with the C oracle and HiGHS alone) and tests/test_gpu_shapes.py (the GPU parity checks).
A plain helper module, like tests/bounds_cases.py, whose slot_template it generalises."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from tests import bounds_cases as BC

N_SCEN = 300              # scenarios per GPU case: no multiple of 64 or 256
N_TRAIN = 512             # the pool's training sample
SEED_VALUES, SEED_TRAIN = 1, 2
# The basis is computed and V is built at X[0]; the pool is refreshed at X[1], a tenth of the way to
# X_FAR.  At X_FAR itself the 512 training solves of the larger templates take 20 to 100 pivots each
# (n: 33 on the GPU) and their eta files outgrow the refresh's first arena of 4096 entries per
# training scenario: the refresh then solves them again with a larger arena (one GPU case does
# that on purpose).  At X[1] they take 2 to 12 pivots (oracle, from the primary basis).
X_FAR = np.array([0.9, 0.4, 0.6, 0.1])
X = [np.array([0.5, 1.0, 0.2, 0.7]), np.array([0.54, 0.94, 0.24, 0.64])]
PENALTY = 50.0
# the environment that requests each of the cut's MFMA passes (the pass values of cut_pass_kind):
# 2 integer limbs, 1 fp32, 0 fp64; the device may still fall back (fp32 range, non-finite deltas)
PASS_ENV = {2: dict(TWOSD_CUT_F32="1", TWOSD_CUT_I8="1"), 1: dict(TWOSD_CUT_F32="1", TWOSD_CUT_I8="0"),
            0: dict(TWOSD_CUT_F32="0", TWOSD_CUT_I8="1")}


def synth_template(m2, ncols, k, seed, senses="EGL", neg_costs=True, amp=1.0):
    """A complete-recourse template with n2 + m2 == ncols exactly.

    Rows cycle through `senses`.  Every 'E' row has +e_i and -e_i penalty columns at cost 50, every
    'G' row +e_i, every 'L' row -e_i, so every rhs is feasible.  The other (structural) columns
    have min(4, m2) nonzeros each.  q = A' pi0 + slack (slack > 0) for a pi0 with |pi0| <= 1 whose
    signs fit the rows ('G' >= 0, 'L' <= 0): pi0 is dual feasible, so every LP is bounded.  Some
    of these q are negative; neg_costs=False lifts them to >= 0.05 (a larger slack), which is what
    the oracle's solve_from_slack needs.  The k random rhs rows take r[rows] + U(-amp, amp)."""
    rng = np.random.default_rng(seed)
    sense = [senses[i % len(senses)] for i in range(m2)]
    npen = sum(2 if s == "E" else 1 for s in sense)
    n2 = ncols - m2
    nA = n2 - npen
    assert nA >= 0 and 1 <= k <= m2, (m2, ncols, k, npen)
    nz = min(4, m2)
    A = np.zeros((m2, nA))
    for j in range(nA):
        i = rng.choice(m2, size=nz, replace=False)
        A[i, j] = rng.uniform(0.5, 2.0, size=nz) * rng.choice([-1.0, 1.0], size=nz)
    P = np.zeros((m2, npen))
    c = 0
    for i, s in enumerate(sense):
        if s in "EG":
            P[i, c] = 1.0
            c += 1
        if s in "EL":
            P[i, c] = -1.0
            c += 1
    W = np.hstack([A, P])
    pi0 = rng.uniform(-1.0, 1.0, size=m2)
    for i, s in enumerate(sense):
        if s == "G":
            pi0[i] = abs(pi0[i])
        elif s == "L":
            pi0[i] = -abs(pi0[i])
    qA = A.T @ pi0 + rng.uniform(0.5, 2.0, size=nA)
    if not neg_costs:
        qA = np.maximum(qA, 0.05)
    q = np.concatenate([qA, np.full(npen, PENALTY)])
    n1 = len(X[0])
    T = np.zeros((m2, n1))
    for j in range(n1):
        i = rng.choice(m2, size=min(6, m2), replace=False)
        T[i, j] = rng.uniform(-1.0, 1.0, size=len(i))
    r = rng.uniform(-2.0, 2.0, size=m2)
    rows = np.sort(rng.choice(m2, size=k, replace=False)).astype(np.int32)
    lb, ub = np.zeros(n2), np.full(n2, np.inf)
    assert W.shape == (m2, n2) and n2 + m2 == ncols
    return SimpleNamespace(m2=m2, n2=n2, k=k, seed=seed, amp=amp, W=W, T=T, q=q, r=r, sense=sense, rows=rows, lb=lb, ub=ub,
                           n_neg=int((q < 0).sum()), positions=[("RHS", f"r{i}") for i in rows],
                           sp2=BC.stage_problem(W, T, q, r, sense, lb, ub), hp=BC.highs_problem(W, q, sense, lb, ub))


# ---- dispatch values, restated from lp_hyper.hip (hyper_rows_per_lane, hyper_cols_per_lane) and
# cut_common.h / cut_plan.h (kCutKBs, cut_kb_for); the GPU test asserts that every value and every slot edge is covered
HR = [1, 2, 4, 9, 16]
HC = [2, 4, 8, 14, 16, 28, 32, 64]
KBS = [1, 2, 4, 6, 8, 12, 16, 22, 24, 30, 32]


def dispatch(m2, ncols, k):
    R = next(v for v in HR if m2 <= 64 * v)
    C = next(v for v in HC if ncols <= 64 * v)
    k4 = (k + 1 + 3) & ~3
    KB = next(v for v in KBS if 4 * v >= k4)
    return R, C, KB


def pg_supported(m, n, kmax=None):
    """pool_gpu.hip's pg_supported: whether the device pool build's LDS layouts fit (otherwise
    pool_refresh composes on the host).  kmax, the LP kernel's eta capacity, is min(256, 2 m + 32)
    or, where the LDS allows, as much of 2 m + 32 as fits below 1024: the default here is that
    upper end, which gives the same verdict on every template."""
    kmax = max(64, min(1024, 2 * m + 32)) if kmax is None else kmax
    ftran = 8 * 16 * m + 4 * (2 * kmax + 1 + m + 1) + m + 16
    count = 8 * 3 * m + 4 * (3 * m + 1) + (n + m) + 16
    fill = 8 * 2 * m + 4 * (4 * (m + 1) + 2 * m) + (n + m) + 16
    return ftran <= 96 * 1024 and count <= 64 * 1024 and fill <= 64 * 1024 and (m + 63) // 64 <= 64


# id: (m2, n2 + m2, k, seed, amp).  amp was picked from a short ladder (0.005 ... 10) as a value at
# which the oracle alone, started from the optimal basis of scenario 0 at X[0], meets every
# condition that tests/test_synth_cases.py asserts.  The comment of each template gives, over
# its N_SCEN scenarios at X[0]: mean / max oracle pivots (cap min(256, 2 m + 32) / 2), scenarios
# with 0 and with >= 3 pivots, distinct dual vectors, and the negative costs among q.
TEMPLATES = {
    "a": (1, 3, 1, 11, 1.0),          # 0.0 / 0 (17), 300 / 0, 1 dual, 0 negative: the smallest LP, one basis
    "b": (40, 128, 3, 12, 10.0),      # 5.0 / 15 (56), 83 / 196, 38 duals, 9 negative (k = 3 needs the wide rhs)
    "c": (20, 129, 4, 13, 0.7),       # 3.3 / 10 (36), 11 / 211, 34 duals, 15 negative
    "d": (64, 256, 7, 14, 0.3),       # 4.5 / 9 (80), 3 / 249, 69 duals, 31 negative
    "e": (65, 257, 8, 15, 0.3),       # 4.4 / 10 (81), 3 / 277, 44 duals, 30 negative
    "f": (128, 512, 15, 16, 0.3),     # 5.9 / 17 (128), 3 / 258, 187 duals, 43 negative
    "g": (129, 513, 16, 17, 0.3),     # 5.8 / 15 (128), 2 / 279, 100 duals, 44 negative
    "h": (256, 896, 23, 18, 0.1),     # 3.6 / 9 (128), 14 / 192, 46 duals, 74 negative
    "i": (257, 897, 24, 19, 0.1),     # 3.1 / 11 (128), 23 / 152, 76 duals, 67 negative
    "j": (40, 1024, 31, 20, 0.1),     # 3.4 / 12 (56), 3 / 214, 83 duals, 178 negative
    "k": (300, 1025, 32, 21, 0.1),    # 2.1 / 8 (128), 36 / 89, 67 duals, 68 negative
    "l": (576, 1792, 47, 22, 0.05),   # 2.6 / 6 (128), 8 / 145, 98 duals, 100 negative
    "m": (577, 1793, 48, 23, 0.1),    # 3.4 / 8 (128), 3 / 202, 49 duals, 101 negative
    "n": (600, 2048, 63, 24, 0.05),   # 2.9 / 11 (128), 28 / 155, 121 duals, 151 negative
    "o": (640, 2049, 64, 25, 0.1),    # 3.5 / 8 (128), 19 / 204, 50 duals, 117 negative
    "p": (1024, 4096, 127, 26, 0.02),  # 10.6 / 27 (128), 1 / 297, 290 duals, 395 negative
}
# the remaining KB edges (22-top, 24-bottom, 24-top, 30-bottom, 30-top, 32-bottom) on one cheap LP
# shape, (R, C) = (4, 8): dvs and cut checks only.  k = 87: 2.4 / 6 (128), 15 / 131, 65 duals.
KB_EDGE_K = [87, 88, 95, 96, 119, 120]
for _k in KB_EDGE_K:
    # k = 119: 2.0 / 5, 18 / 84, 32 duals at 0.135 (from 0.14 on only scenario 0 keeps the start basis)
    TEMPLATES[f"k{_k}"] = (160, 400, _k, 100 + _k, 0.135 if _k == 119 else 0.2)
MAIN_IDS = list("abcdefghijklmnop")
KB_IDS = [f"k{_k}" for _k in KB_EDGE_K]
# Templates exempt from "some scenarios other than scenario 0 need 0 pivots and some need >= 3".
# a has one basis.  p: with amp <= 0.017 some scenarios keep the start basis, but then 8 to 18 of
# the 300 are near-ties of the cut (duals that differ by less than the tie band), past the 2 % cap;
# at amp = 0.02 one is, and only scenario 0 needs no pivot.
NO_PIVOT_SPREAD = {"a", "p"}

# The start basis on the GPU.  twosd_compute_basis solves scenario 0 on the host (phase 1 + primal
# simplex, these q have negative entries).  Measured on the stand-alone host build (host_basis.cpp,
# -O2, one core): g 0.01 s, m 0.9 s, n 4.9 s (4102 pivots), o 3.1 s (2902 pivots), p 202 s (28253
# pivots).  Templates a..m take that route; n, o and p install the committed optimal head
# (tests/golden/synth_heads.npz, written by tests/golden/make_golden.py synth_heads) with set_basis.
GOLDEN_HEADS = ["n", "o", "p"]


def golden_head(tid):
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synth_heads.npz"))
    return z[tid].astype(np.int32)


@functools.lru_cache(maxsize=None)
def template(tid, neg_costs=True):
    m2, ncols, k, seed, amp = TEMPLATES[tid]
    S = synth_template(m2, ncols, k, seed, neg_costs=neg_costs, amp=amp)
    S.id = tid
    S.dispatch = dispatch(m2, ncols, k)
    return S


def values(S, N=N_SCEN, seed=SEED_VALUES):
    """N scenario values of the k random rhs rows: r[rows] + U(-amp, amp)."""
    return S.r[S.rows] + np.random.default_rng(1000 * S.seed + seed).uniform(-S.amp, S.amp, size=(N, S.k))


def rhs(S, x, vals):
    """b = r_w - T x of every scenario."""
    B = np.tile(S.r - S.T @ x, (len(vals), 1))
    B[:, S.rows] += vals - S.r[S.rows]
    return B


def weights(N=N_SCEN):
    return np.random.default_rng(5).uniform(0.5, 1.5, size=N)


def unique_dual_mask(S, y, B, tol=1e-7):
    """Primal nondegeneracy: #(y_j > tol) + #(inequality rows with |slack| > tol) == m2, so the
    optimal basis and with it the dual vector is uniquely determined."""
    ineq = np.array([s != "E" for s in S.sense])
    slack = y @ S.W.T - B
    return (y > tol).sum(1) + (np.abs(slack[:, ineq]) > tol).sum(1) == S.m2


def start_head(S, x, v0):
    """The optimal basis head of scenario v0 at x, read off the HiGHS solution: the positive
    columns and the slacks (numbered n2 + row) of the inactive inequality rows.  The scenario must
    be primal nondegenerate (asserted), so this is the unique optimal basis, the one any simplex
    route ends at (twosd_compute_basis's phase-1 / primal route for these negative costs)."""
    from oracle import lp_highs
    b = rhs(S, x, v0[None, :])[0]
    st, _, y, _ = lp_highs.solve_rhs(S.hp, b)
    assert st == 0
    slack = S.W @ y - b
    head = [j for j in range(S.n2) if y[j] > 1e-7]
    head += [S.n2 + i for i in range(S.m2) if S.sense[i] != "E" and abs(slack[i]) > 1e-7]
    assert len(head) == S.m2, (S.id, len(head), S.m2)
    return np.array(head, dtype=np.int32)


def oracle_lp(S, head):
    from oracle import cpu
    lp = cpu.CpuLP(S.W, S.q, S.sense)
    assert lp.set_basis(head) <= 1e-7          # dual feasible: the start of a dual simplex
    return lp


def oracle_solve(S, lp, x, vals, nthreads=4):
    """(obj, pi, y, status, pivots) of the oracle's dual simplex from lp's basis."""
    return lp.solve_batch(S.rows, S.r - S.T @ x, vals - S.r[S.rows], want_y=True, nthreads=nthreads)


def distinct_rows(pi, decimals=9):
    return len(np.unique(np.round(pi, decimals), axis=0))


def near_ties(scores):
    """Scenarios whose top-two score gap is <= 1e-9 (1 + |best|)."""
    if scores.shape[1] < 2:
        return 0
    part = np.partition(scores, -2, axis=1)[:, -2:]
    hi, lo = part.max(1), part.min(1)
    return int(((hi - lo) <= 1e-9 * (1 + np.abs(hi))).sum())


def cut_scores(S, Vm, x, vals):
    return (Vm @ (S.r - S.T @ x))[None, :] + (vals - S.r[S.rows]) @ Vm[:, S.rows].T


# ---- random technology-matrix (T) elements on the generated templates ---------------------------------
# The templates above have coef_e == 1 on every element (RHS rows only).  t_variant keeps a template's
# W, q, senses and k -- and with k its (R, C, KB) slots -- and re-lays the k random elements so that about
# half are T entries (coef_e = -x[col]), several of them share a row, and one row is a directed tie.
T_AMP = 0.3               # a T element's value: the template's entry + U(-T_AMP, T_AMP)
T_LP_IDS = ["c", "e", "g"]            # LP + pool + cut
T_CUT_IDS = ["k95", "k96"]            # the cut only: KB 24 top / 30 bottom, two int8 slices
T_LAYOUTS = ["distinct", "shared"]
TIE_COL = 0               # X[0][TIE_COL] == 0.5, a power of two: a / x is exact
TIE_OFFSETS = tuple(round((-1) ** i * 4.37 * 1.35 ** i, 2) for i in range(16))   # component i0 of the appended copies: 4.37 ... -394
TIE_TOP = 128              # the most-picked vertices that get copies
# (template, layout): (seed, amp of the RHS elements, scale of TIE_OFFSETS).  With half of the elements
# on T entries (whose effect on the rhs, |dT x[col]| <= 0.3, is small) and several on one row, fewer
# rows of b vary than in the RHS-only template, so amp is picked again from the ladder, and the seed
# and the scale with it, as values at which the oracle and twosd_ref alone meet every condition that
# tests/test_telement_cases.py asserts.  The scale matters because a copy's rounding residue is seen
# only if it survives the last addition base[v] + t, and depends on the order of the two terms only
# while |offset a| is not far above the partial sum it is added to: larger offsets win the argmax
# the same way in either order and hide the smaller ones.
T_VARIANTS = {
    ("c", "distinct"): (0, 3.0, 1.0), ("c", "shared"): (1, 50.0, 1.0),
    ("e", "distinct"): (0, 1.0, 1.0), ("e", "shared"): (1, 4.0, 1.0),
    ("g", "distinct"): (0, 0.3, 1.0), ("g", "shared"): (0, 0.4, 1.0),
    ("k95", "distinct"): (0, 0.2, 1.0), ("k95", "shared"): (0, 1.0, 16.0),
    ("k96", "distinct"): (0, 0.2, 1.0), ("k96", "shared"): (0, 1.0, 16.0),
}


def t_variant(tid, layout, seed=None, amp=None, tie_scale=None):
    """template(tid) with random T elements.  Returns a namespace like template()'s (same W, q, sense,
    m2, n2, k, dispatch) plus: elems = [(row, col)] in listing order (col -1: RHS), rows / cols (int32, per
    element), positions (names), tmpl (template value per element), xz (the X_Z point), canon (the listing
    indices in the canonical order: ascending row, RHS first, T columns ascending), and for "shared"
    i0 / j0, the directed tie row and its T column.

    "distinct": k elements on the template's k rows, RHS and T alternating, listed by descending row (so
    the restated order is not the listing); the first T element sits on a structural zero of T.
    "shared" (k >= 4): the tie row holds (RHS, T); for k >= 7 one row holds (RHS, T, T) and one (T, T)
    (those three rows take 7 elements: template c, k = 4, has the tie row only); the other elements sit
    on rows of their own, RHS and T alternating; the listing is a seeded shuffle.  The tie row i0 is the
    highest random row (so every other element's term is added before its two), with r[i0] = 0 and
    T[i0, :] = 0 on the variant's copy of the template.
    xz = X[0] with one T element's column at 0.0 (coef = -0.0) and another at -0.3 (coef > 0).
    seed, amp (the RHS elements' amplitude) and tie_scale default to T_VARIANTS[(tid, layout)]."""
    B = template(tid)
    assert layout in T_LAYOUTS and (layout == "distinct" or B.k >= 4)
    cfg = T_VARIANTS[(tid, layout)]
    seed, amp, tie_scale = [c if v is None else v for v, c in zip((seed, amp, tie_scale), cfg)]
    rng = np.random.default_rng(100003 * B.seed + 17 * seed + T_LAYOUTS.index(layout))
    k, n1 = B.k, B.T.shape[1]
    r, T = B.r.copy(), B.T.copy()
    i0 = j0 = None
    if layout == "distinct":
        elems, t = [], 0
        for e, i in enumerate(int(v) for v in B.rows):
            if e % 2 == 0 and k > 1:
                elems.append((i, -1))
                continue
            if t == 0:
                c0 = int(np.flatnonzero(T[i] == 0.0)[0])          # a structural zero of T
            elems.append((i, (c0 + t) % n1))
            t += 1
        elems = elems[::-1]
    else:
        groups, left = [[-1, TIE_COL]], k - 2
        if k >= 7:
            groups += [[-1] + sorted(rng.choice(n1, 2, replace=False).tolist()), sorted(rng.choice(n1, 2, replace=False).tolist())]
            left -= 5
        groups += [[int(1 + rng.integers(n1 - 1))] if e % 2 else [-1] for e in range(left)]
        used = [int(v) for v in B.rows[:len(groups)]]
        i0, j0 = used[-1], TIE_COL
        r[i0] = 0.0
        T[i0, :] = 0.0
        order = [used[-1]] + used[:-1]                            # the tie row, then the shared rows from the lowest row up
        elems = [(i, j) for i, g in zip(order, groups) for j in g]
        elems = [elems[p] for p in rng.permutation(len(elems))]
    assert len(elems) == k == len(set(elems))
    rows = np.array([i for i, _ in elems], dtype=np.int32)
    cols = np.array([j for _, j in elems], dtype=np.int32)
    tmpl = np.array([r[i] if j < 0 else T[i, j] for i, j in elems])
    tcols = [int(j) for j in dict.fromkeys(cols[cols >= 0].tolist())]
    pick = [j for j in tcols if j != j0] + [j for j in tcols if j == j0]
    xz = X[0].copy()
    xz[pick[0]] = 0.0
    if len(pick) > 1:
        xz[pick[1]] = -0.3
    S = SimpleNamespace(m2=B.m2, n2=B.n2, k=k, seed=B.seed, amp=amp, tie_scale=tie_scale, W=B.W, T=T, q=B.q, r=r, sense=B.sense, lb=B.lb, ub=B.ub,
                        id=f"{tid}-{layout}", base_id=tid, layout=layout, dispatch=B.dispatch, elems=elems, rows=rows, cols=cols,
                        tmpl=tmpl, xz=xz, i0=i0, j0=j0, vseed=seed,
                        positions=[("RHS" if j < 0 else f"x{j}", f"r{i}") for i, j in elems],
                        canon=sorted(range(k), key=lambda e: elems[e]),
                        sp2=BC.stage_problem(B.W, T, B.q, r, B.sense, B.lb, B.ub), hp=B.hp)
    # what oracle/twosd_ref.Coefficients reads
    S.osp = SimpleNamespace(r=r, T=T, W=B.W, last_names=[f"x{j}" for j in range(n1)], row_names=[f"r{i}" for i in range(B.m2)])
    return S


def t_relisted(S, perm):
    """S with its elements listed in the order perm (listing indices); t_values(S)[:, perm] are its values."""
    R = SimpleNamespace(**vars(S))
    R.elems = [S.elems[e] for e in perm]
    R.rows, R.cols, R.tmpl = S.rows[perm], S.cols[perm], S.tmpl[perm]
    R.positions = [S.positions[e] for e in perm]
    R.canon = sorted(range(S.k), key=lambda e: R.elems[e])
    return R


def t_xs(S):
    """The x points of the T variants: where V is built, elsewhere, and X_Z."""
    return [("X0", X[0]), ("X1", X[1]), ("XZ", S.xz)]


def t_values(S, N=N_SCEN, seed=SEED_VALUES):
    """N scenario values of the k elements in listing order: r[row] + U(-amp, amp) for an RHS element,
    T[row, col] + U(-T_AMP, T_AMP) for a T element; on the tie row a ~ U(-1, 1) for the RHS element and
    a / X[0][j0] (exact: a power of two) for the T element, so that coef * dv == -a at X[0]."""
    rng = np.random.default_rng(1000 * S.seed + 31 * S.vseed + seed)
    u = rng.uniform(-1.0, 1.0, size=(N, S.k))
    a = rng.uniform(-1.0, 1.0, size=N)
    vals = np.empty((N, S.k))
    for e, (i, j) in enumerate(S.elems):
        if i == S.i0:
            vals[:, e] = a if j < 0 else a / X[0][S.j0]
        else:
            vals[:, e] = S.tmpl[e] + (S.amp if j < 0 else T_AMP) * u[:, S.canon.index(e)]
    return vals


def t_coef(S, x):
    """coef_e(x): 1 for an RHS element, -x[col] for a T element."""
    return np.array([1.0 if j < 0 else -x[j] for _, j in S.elems])


def t_rhs_deltas(S, x, vals):
    """(rows, base, DR) of the oracle LP: b = base + sum_e DR[:, e] e_row(e), base = r - T x, DR = dr for an
    RHS element and -(dT) x[col] for a T element (b = (r + dr) - (T + dT) x)."""
    return S.rows, S.r - S.T @ x, (vals - S.tmpl) * t_coef(S, x)[None, :]


def t_rhs(S, x, vals):
    rows, base, DR = t_rhs_deltas(S, x, vals)
    B = np.tile(base, (len(vals), 1))
    for e, i in enumerate(rows):
        B[:, i] += DR[:, e]
    return B


def t_start_head(S, x, v0):
    """start_head for a T variant: the unique optimal basis of scenario v0 at x (HiGHS)."""
    from oracle import lp_highs
    b = t_rhs(S, x, v0[None, :])[0]
    st, _, y, _ = lp_highs.solve_rhs(S.hp, b)
    assert st == 0
    slack = S.W @ y - b
    head = [j for j in range(S.n2) if y[j] > 1e-7]
    head += [S.n2 + i for i in range(S.m2) if S.sense[i] != "E" and abs(slack[i]) > 1e-7]
    assert len(head) == S.m2, (S.id, len(head), S.m2)
    return np.array(head, dtype=np.int32)


def t_oracle_solve(S, lp, x, vals, nthreads=4):
    rows, base, DR = t_rhs_deltas(S, x, vals)
    return lp.solve_batch(rows, base, DR, want_y=True, nthreads=nthreads)


def t_scores(S, Vm, x, vals):
    """Scores of every (scenario, vertex) to rounding (the near-tie count, not a decision)."""
    _, base, DR = t_rhs_deltas(S, x, vals)
    return (Vm @ base)[None, :] + DR @ Vm[:, S.rows].T


def t_ref_deltas(S, vals):
    """(Coefficients, [delta_coefficients of every scenario]) of oracle/twosd_ref.py."""
    from oracle import twosd_ref
    coef = twosd_ref.Coefficients(S.osp)
    return coef, [twosd_ref.delta_coefficients(coef, list(zip(S.positions, v))) for v in vals]


def t_with_tie_copies(S, Vm, picks):
    """Vm with copies of the TIE_TOP most-picked vertices appended, each changed only in component i0 by
    one of TIE_OFFSETS: at X[0] a copy ties its original exactly in real arithmetic (row i0's base is 0
    and its two terms cancel), so rounding and the order of the two terms decide the pick."""
    top = np.argsort(-np.bincount(picks, minlength=len(Vm)), kind="stable")[:TIE_TOP]
    copies = []
    for off in TIE_OFFSETS:
        off = S.tie_scale * off
        c = Vm[top].copy()
        c[:, S.i0] += off
        copies.append(c)
    return np.vstack([Vm] + copies)


def t_reversed_within_rows(S):
    """The element listing [(row, col)] in the canonical order with every row's elements reversed."""
    return sorted(S.elems, key=lambda p: (p[0], -p[1]))
