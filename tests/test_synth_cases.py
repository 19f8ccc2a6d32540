"""The conditions on the inputs of tests/test_gpu_shapes.py, proved with the C oracle and HiGHS
alone (no GPU): every generated template of tests/synth_cases.py has the shape and structure it
claims, sits on the dispatch edge it is meant for, and gives the GPU test something to get wrong
(many distinct duals, scenarios with and without pivots, uniquely determined duals, few cut
near-ties) within the kernel's pivot budget.  Asserted directly, so that a changed seed or amp
cannot silently hollow out a GPU case."""
import functools

import numpy as np
import pytest

from tests import synth_cases as SC

ALL_IDS = SC.MAIN_IDS + SC.KB_IDS


@functools.lru_cache(maxsize=None)
def _run(tid):
    """The oracle on the N_SCEN scenarios at X[0], from the optimal basis of scenario 0."""
    from oracle import twosd_ref
    S = SC.template(tid)
    vals = SC.values(S)
    head = SC.golden_head(tid) if tid in SC.GOLDEN_HEADS else SC.start_head(S, SC.X[0], vals[0])
    lp = SC.oracle_lp(S, head)
    obj, pi, y, st, it = SC.oracle_solve(S, lp, SC.X[0], vals)
    V = twosd_ref.DualVertexSet()
    V.push_batch(pi[st == 0])
    return S, vals, head, lp, obj, pi, y, st, it, V.matrix(S.m2)


@pytest.mark.parametrize("tid", ALL_IDS)
def test_template_structure(tid):
    m2, ncols, k, seed, amp = SC.TEMPLATES[tid]
    S = SC.template(tid)
    assert S.W.shape == (m2, ncols - m2) and S.n2 + S.m2 == ncols and len(S.rows) == k == len(set(S.rows.tolist()))
    nnz = (S.W != 0).sum(0)
    pen = np.nonzero(S.q == SC.PENALTY)[0]
    struct = np.nonzero(S.q != SC.PENALTY)[0]
    assert (nnz[struct] == min(4, m2)).all() and (nnz[pen] == 1).all()
    for i, s in enumerate(S.sense):                      # complete recourse
        col = S.W[i, pen]
        assert ((col == 1.0).sum(), (col == -1.0).sum()) == {"E": (1, 1), "G": (1, 0), "L": (0, 1)}[s]
    if tid != "a":
        assert S.n_neg > 0                               # the host phase-1 / primal route
    vals = SC.values(S)
    assert vals.shape == (SC.N_SCEN, k) and np.abs(vals - S.r[S.rows]).max() <= amp
    assert SC.N_SCEN % 64 and SC.N_SCEN % 256            # a ragged last wave and block


def test_nonnegative_costs_variant_solves_from_slack():
    from oracle import cpu
    S = SC.template("e", neg_costs=False)
    assert (S.q >= 0).all() and S.W.shape == SC.template("e").W.shape
    st, obj, head, _ = cpu.CpuLP(S.W, S.q, S.sense).solve_from_slack(SC.rhs(S, SC.X[0], SC.values(S)[:1])[0])
    assert st == 0 and len(head) == S.m2


def test_every_dispatch_value_and_slot_edge_is_covered():
    shapes = [SC.TEMPLATES[t][:3] for t in ALL_IDS]
    disp = [SC.dispatch(*s) for s in shapes]
    assert {d[0] for d in disp} == set(SC.HR) and {d[1] for d in disp} == set(SC.HC) and {d[2] for d in disp} == set(SC.KBS)
    ms = {s[0] for s in shapes}
    ncs = {s[1] for s in shapes}
    k1 = {s[2] + 1 for s in shapes}
    for prev, v in zip([None] + SC.HR, SC.HR):
        assert 64 * v in ms and (prev is None or 64 * prev + 1 in ms), v
    for prev, v in zip([None] + SC.HC, SC.HC):
        assert 64 * v in ncs and (prev is None or 64 * prev + 1 in ncs), v
    for prev, v in zip([None] + SC.KBS, SC.KBS):
        assert 4 * v in k1 and (prev is None or 4 * prev + 1 in k1), v
    # the LP checks run on the main templates: they alone cover every (R, C) value and edge
    main = [SC.TEMPLATES[t][:3] for t in SC.MAIN_IDS]
    assert {SC.dispatch(*s)[0] for s in main} == set(SC.HR) and {SC.dispatch(*s)[1] for s in main} == set(SC.HC)
    # the device pool build fits every template but the 1024-row one
    assert [t for t in SC.MAIN_IDS if not SC.pg_supported(SC.TEMPLATES[t][0], SC.TEMPLATES[t][1] - SC.TEMPLATES[t][0])] == ["p"]


@pytest.mark.parametrize("tid", ALL_IDS)
def test_conditions_on_the_inputs(tid):
    from oracle import lp_highs
    S, vals, head, lp, obj, pi, y, st, it, Vm = _run(tid)
    N = SC.N_SCEN
    assert (st == 0).all(), np.bincount(st)
    B = SC.rhs(S, SC.X[0], vals)
    for s in range(0, N, N // 8):
        hst, hobj, _, _ = lp_highs.solve_rhs(S.hp, B[s])
        assert hst == 0 and abs(hobj - obj[s]) <= 1e-8 * (1 + abs(hobj)), (s, hobj, obj[s])
    distinct = SC.distinct_rows(pi)
    zero, ge3 = int((it == 0).sum()), int((it >= 3).sum())
    unique = SC.unique_dual_mask(S, y, B)
    ties = [SC.near_ties(SC.cut_scores(S, Vm, x, vals)) for x in SC.X]
    print(f"{tid}: pivots mean {it.mean():.1f} max {it.max()}, zero {zero}, >=3 {ge3}, distinct duals {distinct}, |V| {len(Vm)}, "
          f"unique {unique.mean():.3f}, near-ties {ties}")
    if tid != "a":
        assert distinct >= 30
    assert it.max() <= min(256, 2 * S.m2 + 32) // 2
    assert it[0] == 0                                    # the start basis is scenario 0's optimal one
    if tid not in SC.NO_PIVOT_SPREAD:
        assert zero >= 2 and ge3 >= 1                    # some besides scenario 0 keep the start basis
    assert unique.mean() >= 0.9
    assert max(ties) <= 0.02 * N
    # the pool part of the GPU test also solves the training sample at X[1] from this basis
    tr = SC.values(S, SC.N_TRAIN, SC.SEED_TRAIN)
    for v in (vals, tr):
        _, _, _, st1, it1 = SC.oracle_solve(S, lp, SC.X[1], v)
        assert (st1 == 0).all() and it1.max() < min(256, 2 * S.m2 + 32)


@pytest.mark.parametrize("tid", SC.GOLDEN_HEADS)
def test_committed_heads_are_the_optimal_bases(tid):
    """tests/golden/synth_heads.npz holds what make_golden.py's synth_heads writes: the optimal
    basis of scenario 0 at X[0] (the templates whose host setup solve takes seconds to minutes;
    the measured times are in tests/synth_cases.py)."""
    S = SC.template(tid)
    head = SC.golden_head(tid)
    assert sorted(head.tolist()) == sorted(SC.start_head(S, SC.X[0], SC.values(S)[0]).tolist())
    _, _, _, st, it = SC.oracle_solve(S, SC.oracle_lp(S, head), SC.X[0], SC.values(S)[:1])
    assert st[0] == 0 and it[0] == 0
