"""The conditions on the inputs of tests/test_gpu_telements.py, proved with the C oracle, HiGHS and
oracle/twosd_ref.py alone (no GPU): every T variant of tests/synth_cases.py (t_variant: random
technology-matrix elements, coef_e = -x[col], on the generated templates) has the layout it claims,
solves at the three x points, has many distinct duals and few cut near-ties, and -- for the "shared"
layout -- its directed tie row makes the pick depend on the order of a row's terms, so that a device
that follows the caller's listing instead of the canonical order cannot pass the GPU test."""
import functools

import numpy as np
import pytest

from tests import synth_cases as SC

CASES = [(t, lay) for t in SC.T_LP_IDS + SC.T_CUT_IDS for lay in SC.T_LAYOUTS]
# Distinct duals at X[0]: 30 as in the RHS-only sweep, and for template c the 34 its RHS-only run reaches
# (synth_cases).  c-shared cannot reach that: of its k = 4 elements two sit on the tie row, whose terms
# cancel at X[0], so b varies with one RHS element and one T element (|dT x| <= 0.3) only -- nearly a
# one-parameter family of right-hand sides, whose optimal bases are the breakpoints of one parametric
# LP.  One RHS row of c alone gives 5 / 11 / 22 distinct duals at amp 3 / 10 / 30 and the penalty
# columns (cost 50) end the growth; the variant reaches 25 to 28 over seeds 0..5 at amp 40 to 70.
MIN_DUALS = {("c", "distinct"): 34, ("c", "shared"): 24}


@functools.lru_cache(maxsize=None)
def run(tid, layout):
    """The oracle on the N_SCEN scenarios at X[0], from the optimal basis of scenario 0, and the vertex
    set of its duals.  Shared with the GPU tests (the reference side is computed once)."""
    from oracle import twosd_ref
    S = SC.t_variant(tid, layout)
    vals = SC.t_values(S)
    B = SC.template(tid)                                   # the RHS-only template's start basis: dual feasible for the same W, q
    head = SC.start_head(B, SC.X[0], SC.values(B)[0])
    lp = SC.oracle_lp(S, head)
    obj, pi, y, st, it = SC.t_oracle_solve(S, lp, SC.X[0], vals)
    V = twosd_ref.DualVertexSet()
    V.push_batch(pi[st == 0])
    return S, vals, head, lp, obj, pi, st, it, V.matrix(S.m2)


@pytest.mark.parametrize("tid,layout", CASES)
def test_layout_has_what_it_claims(tid, layout):
    S = SC.t_variant(tid, layout)
    B = SC.template(tid)
    assert S.k == B.k and S.dispatch == B.dispatch and S.W is B.W and len(set(S.elems)) == S.k
    nT = int((S.cols >= 0).sum())
    assert S.k // 2 - 1 <= nT <= S.k // 2 + 2 and nT >= 2                   # about half are T entries
    assert any(j >= 0 and S.T[i, j] == 0.0 for i, j in S.elems)              # a structural zero of T
    per_row = np.bincount(S.rows)
    kinds = {tuple(sorted(-1 if j < 0 else 0 for i2, j in S.elems if i2 == i)) for i in set(S.rows.tolist())}
    if layout == "distinct":
        assert per_row.max() == 1 and S.elems != sorted(S.elems)
    else:
        # rows with (RHS, T), (RHS, T, T) and (T, T) take 7 elements: template c (k = 4) has the tie row
        # (RHS, T) and an RHS and a T element on rows of their own
        assert (-1, 0) in kinds and (((-1, 0, 0) in kinds and (0, 0) in kinds) == (S.k >= 7))
        assert per_row.max() == (3 if S.k >= 7 else 2)
        assert [S.elems[e] for e in S.canon] != S.elems                      # the listing is not the canonical order
        assert S.r[S.i0] == 0.0 and not S.T[S.i0].any() and S.i0 == S.rows.max()
        assert sorted(j for i, j in S.elems if i == S.i0) == [-1, S.j0]
        vals = SC.t_values(S)
        c = SC.t_coef(S, SC.X[0])
        e_r, e_t = S.elems.index((S.i0, -1)), S.elems.index((S.i0, S.j0))
        assert np.array_equal(c[e_t] * (vals[:, e_t] - S.tmpl[e_t]), -(vals[:, e_r] - S.tmpl[e_r]))   # exact cancellation
    cz = SC.t_coef(S, S.xz)
    assert ((cz == 0.0) & np.signbit(cz)).any() and (cz[S.cols >= 0] > 0).any()     # coef -0.0 and coef > 0 at X_Z
    vals = SC.t_values(S)
    assert vals.shape == (SC.N_SCEN, S.k)
    # relisting permutes the columns and nothing else (a shared row's terms are added in another order)
    perm = list(reversed(range(S.k)))
    R = SC.t_relisted(S, perm)
    assert sorted(R.elems) == sorted(S.elems) and [R.elems[e] for e in R.canon] == [S.elems[e] for e in S.canon]
    np.testing.assert_allclose(SC.t_rhs(R, SC.X[1], vals[:, perm]), SC.t_rhs(S, SC.X[1], vals), rtol=0, atol=1e-14)


@pytest.mark.parametrize("tid,layout", CASES)
def test_conditions_on_the_inputs(tid, layout):
    from oracle import lp_highs, twosd_ref
    S, vals, head, lp, obj, pi, st, it, Vm = run(tid, layout)
    N = SC.N_SCEN
    assert (st == 0).all(), np.bincount(st)
    assert it.max() < min(256, 2 * S.m2 + 32)
    for name, x in SC.t_xs(S):                             # all LPs optimal at the three x; HiGHS agrees
        o, _, _, s1, it1 = SC.t_oracle_solve(S, lp, x, vals)
        assert (s1 == 0).all() and it1.max() < min(256, 2 * S.m2 + 32), (name, np.bincount(s1))
        Bx = SC.t_rhs(S, x, vals)
        for s in range(0, N, N // 8):
            hst, hobj, _, _ = lp_highs.solve_rhs(S.hp, Bx[s])
            assert hst == 0 and abs(hobj - o[s]) <= 1e-8 * (1 + abs(hobj)), (name, s, hobj, o[s])
    distinct = SC.distinct_rows(pi)
    ties = [SC.near_ties(SC.t_scores(S, Vm, x, vals)) for _, x in SC.t_xs(S)]
    print(f"{S.id}: pivots mean {it.mean():.1f} max {it.max()}, distinct duals {distinct}, |V| {len(Vm)}, near-ties {ties}")
    assert distinct >= MIN_DUALS.get((tid, layout), 30)
    assert max(ties) <= 0.02 * N                           # outside the directed vertices
    if layout == "shared":
        coef, deltas = SC.t_ref_deltas(S, vals)
        _, picks = twosd_ref.argmax_procedure(coef, deltas, SC.X[0], Vm, 0.0)
        Vt = SC.t_with_tie_copies(S, Vm, picks)
        _, canon = twosd_ref.argmax_procedure(coef, deltas, SC.X[0], Vt, 0.0)
        _, rev = twosd_ref.argmax_procedure(coef, deltas, SC.X[0], Vt, 0.0, order=SC.t_reversed_within_rows(S))
        _, lst = twosd_ref.argmax_procedure(coef, deltas, SC.X[0], Vt, 0.0, order=S.elems)
        differ = int((canon != rev).sum())
        print(f"{S.id}: canonical and reversed within-row order pick differently on {differ} of {N} scenarios "
              f"(the listing's order: {int((canon != lst).sum())}); {int((canon >= len(Vm)).sum())} pick a copy")
        assert differ >= 0.03 * N
        # the canonical order given as a listing is the default
        _, same = twosd_ref.argmax_procedure(coef, deltas, SC.X[0], Vt, 0.0, order=sorted(S.elems))
        np.testing.assert_array_equal(same, canon)
