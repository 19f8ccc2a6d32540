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
# cut_kernel.hip (kb_for); the GPU test asserts that every value and every slot edge is covered
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
