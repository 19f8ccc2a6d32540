"""Random technology-matrix (T) elements, coef_e(x) = -x[col], through every kernel that takes the
per-element factor: the LP (full and lean), the pool build / refresh / selection, the cut's three MFMA
passes and its fixup, the sharded partials, the bootstrap re-formation, the sampler and the stream
moments -- on the T variants of the generated templates (tests/synth_cases.py t_variant;
tests/test_telement_cases.py proves without a GPU that the inputs have what these checks need).

What the RHS-only inputs (coef_e == 1) cannot show and these do: a per-x copy of coef_e that is stale
after x changed (solve / cut at x, at another x, at x again: the same bits), a folded factor other
than 1 in the fp32 and integer passes (also coef = -0.0 and coef > 0 at X_Z), several elements on one
row, whose order within the row decides rounding-level ties (the canonical order -- ascending row, RHS
first, then T columns ascending -- whatever the caller's listing), and a position listed twice.

References: the C dual simplex and HiGHS for the LP, oracle/twosd_ref.py (build_sasa_cut, exact picks,
no near-tie exemption) for the cut, tests/boot_ref.py, oracle.cpu.sample_deltas and tests/vr_ref.py.
The tolerances are the suite's: objectives 1e-9 (HiGHS 1e-8), alpha / beta 1e-8, weight_mark 1e-15, host
against device pool 1e-12, NORMAL draws 1e-12, stream moments as in tests/test_gpu_evaluate_ci.py."""
import functools
import os

import numpy as np
import pytest

from tests import boot_ref as BR
from tests import synth_cases as SC
from tests import vr_ref as VR

pytestmark = pytest.mark.gpu

N = SC.N_SCEN
CUT_IDS = SC.T_LP_IDS + SC.T_CUT_IDS


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ctx(S, vals):
    """A context on the variant with the optimal basis of scenario 0 at X[0] as the primary basis."""
    from sqlp_amd import twosd
    ctx = twosd.SDContext(S.sp2, positions=S.positions)
    assert (ctx.m_lp, ctx.n_lp, ctx.k) == (S.m2, S.n2, S.k)
    np.testing.assert_array_equal(ctx.rows, S.rows)
    np.testing.assert_array_equal(ctx.cols, S.cols)
    np.testing.assert_array_equal(ctx.template_values, S.tmpl)
    ctx.compute_basis(SC.X[0], vals[0])
    return ctx


def _oracle_lp(S, ctx):
    from oracle import cpu
    lp = cpu.CpuLP(S.W, S.q, S.sense)
    lp.set_basis(ctx.get_basis())
    return lp


@functools.lru_cache(maxsize=None)
def _ref(tid, layout):
    """(S, values, weights, Coefficients, deltas) of a variant: the reference side, computed once."""
    S = SC.t_variant(tid, layout)
    vals = SC.t_values(S)
    vals.setflags(write=False)
    coef, deltas = SC.t_ref_deltas(S, vals)
    return S, vals, SC.weights(), coef, deltas


# ---- 1. LP at three x on one context, then with a pool --------------------------------------------------
@pytest.mark.parametrize("layout", SC.T_LAYOUTS)
@pytest.mark.parametrize("tid", SC.T_LP_IDS)
def test_lp_at_three_x_on_one_context(tid, layout, monkeypatch):
    from oracle import lp_highs, twosd_ref
    from sqlp_amd import twosd
    S, vals, _, coef, deltas = _ref(tid, layout)
    ctx = _ctx(S, vals)
    lp = _oracle_lp(S, ctx)
    seq = [("X0", SC.X[0]), ("XZ", S.xz), ("X1", SC.X[1]), ("X0", SC.X[0])]
    runs, worst = [], 0.0
    for name, x in seq:
        obj, _, pi, st = ctx.solve_values(x, vals, want_pi=True)
        assert (st == 0).all(), (name, np.bincount(st))
        lean, _, _, st2 = ctx.solve_values(x, vals, want_pi=False)                 # the lean kernel
        assert (st2 == 0).all()
        np.testing.assert_array_equal(lean, obj)
        o_obj, _, _, o_st, _ = SC.t_oracle_solve(S, lp, x, vals)
        assert (o_st == 0).all()
        worst = max(worst, float((np.abs(obj - o_obj) / (1 + np.abs(o_obj))).max()))
        np.testing.assert_allclose(obj, o_obj, rtol=1e-9, atol=1e-9)
        B = SC.t_rhs(S, x, vals)
        for s in range(0, N, 16):
            hst, hobj, _, _ = lp_highs.solve_rhs(S.hp, B[s])
            assert hst == 0 and abs(hobj - obj[s]) <= 1e-8 * (1 + abs(hobj)), (name, s, hobj, obj[s])
        for s in range(N):                                                         # strong duality
            assert abs(twosd_ref.eval_dual(coef, deltas[s], x, pi[s]) - obj[s]) <= 1e-9 * (1 + abs(obj[s])), (name, s)
        runs.append((obj, st, pi))
    for a, b in zip(runs[0], runs[3]):                                             # at X[0] again: the same bits
        np.testing.assert_array_equal(a, b)
    print(f"TELEM lp {S.id}: worst objective error {worst:.3e} relative")
    ref_z, ref_0 = runs[1][0], runs[0][0]
    # pool: built at X[0], refreshed at X[1], then solves at X_Z and X[0]; host against device build
    got = {}
    for mode in ("host", "device"):
        if mode == "host":
            monkeypatch.setenv("TWOSD_REFRESH_HOST", "1")
        else:
            monkeypatch.delenv("TWOSD_REFRESH_HOST", raising=False)
        pc = _ctx(S, vals)
        tr = twosd.sdEpigraph(pc, 1.0, 0.0)
        twosd.add_scenarios(tr, SC.t_values(S, SC.N_TRAIN, SC.SEED_TRAIN))
        size = pc.pool_build(tr, SC.X[0], 0, SC.N_TRAIN, 16)
        assert 1 <= size <= 16
        P = pc.pool_refresh(tr, SC.X[1], 0, SC.N_TRAIN, 64)
        assert 1 < P <= 64
        out = []
        for x, ref in ((S.xz, ref_z), (SC.X[0], ref_0)):
            o, _, _, st = pc.solve_values(x, vals, want_pi=False)
            assert (st == 0).all()
            picks = pc.last_pool_picks(N)
            assert picks.min() >= 0 and picks.max() < P
            np.testing.assert_allclose(o, ref, rtol=1e-9, atol=1e-9)
            out.append(o)
        got[mode] = (P, [pc.pool_get(p) for p in range(P)], out)
    assert got["host"][0] == got["device"][0]
    for a, b in zip(got["host"][1], got["device"][1]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(got["host"][2], got["device"][2]):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)


# ---- 2. cut -------------------------------------------------------------------------------------------------
def _vertices(ctx, vals):
    """The vertex set of the LP duals at X[0] (the context's one set, left holding them)."""
    from sqlp_amd import twosd
    _, _, pi, st = ctx.solve_values(SC.X[0], vals, want_pi=True)
    assert (st == 0).all()
    V = twosd.sdDualVertexSet(ctx)
    V.push_batch(pi)
    return V, V.matrix()


def _check_cut(S, ctx, epi, Vm, w, coef, deltas, tag):
    """Every x, both tie rules, the three passes requested: exact picks, alpha / beta 1e-8, weight_mark
    1e-15 against twosd_ref.build_sasa_cut in the canonical element order.  Returns the worst alpha error
    and, per pass requested and x, the pass that ran and the rows handed to the fixup."""
    from oracle import twosd_ref
    from sqlp_amd import twosd
    worst, record = 0.0, {}
    for name, x in SC.t_xs(S):
        for tie_rel in (0.0, 1e-12):
            a, b, wm, omv, oma = twosd_ref.build_sasa_cut(coef, deltas, w, x, Vm, tie_rel=tie_rel)
            for kind in (2, 1, 0):
                with _env(**SC.PASS_ENV[kind]):
                    cut, mv, ma = twosd._build_cut(epi, x, tie_rel, want_argmax=True)
                    ran = ctx.cut_pass_kind()[0]
                    fixed = ctx.cut_stats()[0]
                # the pass requested runs; at X_Z (coef = -0.0 on one element, > 0 on another) the device may
                # fall back to a wider pass (recorded below; on the MI355X none did)
                allowed = {kind} if name != "XZ" else set(range(kind + 1))
                assert ran in allowed, (tag, name, kind, ran)
                record[(kind, name)] = (ran, fixed)
                assert cut.weight_mark == pytest.approx(wm, rel=1e-15)
                bad = np.nonzero(ma != oma)[0]
                assert bad.size == 0, (tag, name, tie_rel, kind, bad[:8].tolist(), ma[bad[:8]].tolist(), oma[bad[:8]].tolist())
                np.testing.assert_allclose(mv, omv, rtol=1e-10, atol=1e-9)
                worst = max(worst, abs(cut.alpha - a) / (1 + abs(a)))
                assert cut.alpha == pytest.approx(a, rel=1e-8, abs=1e-8)
                np.testing.assert_allclose(cut.beta, b, rtol=1e-8, atol=1e-8 * (1 + np.abs(b).max()))
    print(f"TELEM cut {tag}: |V| {len(Vm)}, worst alpha error {worst:.3e} relative, (pass requested, x): (pass run, rows to the fixup) "
          f"{ {k: v for k, v in sorted(record.items())} }")
    return worst, record


def _same_bits_when_x_returns(S, epi):
    """X[0], X_Z, X[0] on one epigraph: the first and the third cut are bit-identical."""
    from sqlp_amd import twosd
    out = [twosd._build_cut(epi, x, 0.0, want_argmax=True) for x in (SC.X[0], S.xz, SC.X[0])]
    (c0, mv0, ma0), (cz, _, _), (c2, mv2, ma2) = out
    np.testing.assert_array_equal(ma0, ma2)
    np.testing.assert_array_equal(mv0, mv2)
    assert c0.alpha == c2.alpha and np.array_equal(c0.beta, c2.beta)
    assert cz.alpha != c0.alpha                                                   # X_Z gives another cut


@pytest.mark.parametrize("tid", CUT_IDS)
def test_cut_distinct_rows(tid):
    from sqlp_amd import twosd
    S, vals, w, coef, deltas = _ref(tid, "distinct")
    ctx = _ctx(S, vals)
    V, Vm = _vertices(ctx, vals)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals, w)
    _check_cut(S, ctx, epi, Vm, w, coef, deltas, S.id)
    _same_bits_when_x_returns(S, epi)


@functools.lru_cache(maxsize=None)
def _tie_vertices(tid):
    """The "shared" variant's vertex set: the LP duals at X[0] (from the device) plus the directed tie
    copies of the most-picked vertices (picked by the reference in the canonical order)."""
    from oracle import twosd_ref
    S, vals, w, coef, deltas = _ref(tid, "shared")
    ctx = _ctx(S, vals)
    _, Vm = _vertices(ctx, vals)
    head = ctx.get_basis()
    ctx.close()
    _, picks = twosd_ref.argmax_procedure(coef, deltas, SC.X[0], Vm, 0.0)
    Vt = SC.t_with_tie_copies(S, Vm, picks)
    Vt.setflags(write=False)
    return Vt, head


def _shared_ctx(R, rvals, w, Vt, head):
    from sqlp_amd import twosd
    ctx = twosd.SDContext(R.sp2, positions=R.positions)
    ctx.set_basis(head)
    V = twosd.sdDualVertexSet(ctx)
    V.push_batch(Vt)
    assert len(V) == len(Vt)
    np.testing.assert_array_equal(V.matrix(), Vt)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, rvals, w)
    return ctx, V, epi


@pytest.mark.parametrize("tid", CUT_IDS)
def test_cut_shared_rows(tid):
    S, vals, w, coef, deltas = _ref(tid, "shared")
    Vt, head = _tie_vertices(tid)
    ctx, V, epi = _shared_ctx(S, vals, w, Vt, head)
    _check_cut(S, ctx, epi, Vt, w, coef, deltas, S.id)
    _same_bits_when_x_returns(S, epi)


@pytest.mark.parametrize("tid", CUT_IDS)
def test_cut_does_not_depend_on_the_listing(tid):
    """Three contexts whose positions are listed canonically, reversed within every row, and shuffled (the
    variant's own listing), the value columns permuted to match: identical picks, the reference's in the
    canonical order.  tests/test_telement_cases.py proves that on at least 3 % of the scenarios the pick
    differs between the canonical and the reversed order, so a device that follows the listing fails."""
    from oracle import twosd_ref
    from sqlp_amd import twosd
    S, vals, w, coef, deltas = _ref(tid, "shared")
    Vt, head = _tie_vertices(tid)
    a, b, wm, omv, oma = twosd_ref.build_sasa_cut(coef, deltas, w, SC.X[0], Vt, tie_rel=0.0)
    rev = SC.t_reversed_within_rows(S)
    listings = {"canonical": list(S.canon), "reversed": [S.elems.index(p) for p in rev], "shuffled": list(range(S.k))}
    got = {}
    for name, perm in listings.items():
        R = SC.t_relisted(S, perm)
        ctx, V, epi = _shared_ctx(R, vals[:, perm], w, Vt, head)
        cut, mv, ma = twosd._build_cut(epi, SC.X[0], 0.0, want_argmax=True)
        got[name] = ma
        print(f"TELEM listing {S.id} {name}: {int((ma != oma).sum())} of {N} picks differ from the canonical reference")
        assert cut.alpha == pytest.approx(a, rel=1e-8, abs=1e-8)
        np.testing.assert_allclose(cut.beta, b, rtol=1e-8, atol=1e-8 * (1 + np.abs(b).max()))
        ctx.close()
    for name in listings:
        np.testing.assert_array_equal(got[name], oma, err_msg=name)


def test_sharded_partials_equal_single_cut():
    """twosd_cut_partial on two scenario shards + host sum + finalize == the single cut, with T elements
    on shared rows (beta includes the -sum_e S_e e_col(e) terms): tests/test_gpu_cut.py's twin."""
    import torch
    from sqlp_amd import twosd
    S, vals, w, coef, deltas = _ref("e", "shared")
    Vt, head = _tie_vertices("e")
    ctx, V, full = _shared_ctx(S, vals, w, Vt, head)
    for x in (SC.X[0], S.xz):
        ref = twosd.build_sasa_cut(full, x, V, tie_rel=0.0)
        halves = [twosd.sdEpigraph(ctx, 1.0, 0.0) for _ in range(2)]
        twosd.add_scenarios(halves[0], vals[:130], w[:130])
        twosd.add_scenarios(halves[1], vals[130:], w[130:])
        nu, nf = ctx.cut_partial_len()
        dev = torch.device("cuda", 0)
        H = [torch.zeros(nu, dtype=torch.int64, device=dev) for _ in range(2)]
        Sm = [torch.zeros(nf, dtype=torch.float64, device=dev) for _ in range(2)]
        hist1 = torch.zeros(nu, dtype=torch.int64, device=dev)
        sums1 = torch.zeros(nf, dtype=torch.float64, device=dev)
        ctx.cut_partial(full, x, 0.0, w.sum(), hist1.data_ptr(), sums1.data_ptr())
        for e in range(2):
            ctx.cut_partial(halves[e], x, 0.0, w.sum(), H[e].data_ptr(), Sm[e].data_ptr())
        torch.cuda.synchronize()
        hist, sums = H[0] + H[1], Sm[0] + Sm[1]
        assert torch.equal(hist, hist1)
        a, b = ctx.cut_finalize(x, hist.data_ptr(), sums.data_ptr())
        assert a == pytest.approx(ref.alpha, rel=1e-12)
        np.testing.assert_allclose(b, ref.beta, rtol=1e-12, atol=1e-12)


def test_bootstrap_reform_with_shared_rows():
    """reform_cuts over the kept picks of a cut of c-shared against tests/boot_ref.py: the replicate
    count (33, index offset 1000) and the tolerance of tests/test_gpu_bootstrap.py's random-T case."""
    from sqlp_amd import twosd
    from tests.test_gpu_bootstrap import _close, _template_arrays
    S, vals, w, coef, deltas = _ref("c", "shared")
    Vt, head = _tie_vertices("c")
    ctx, V, epi = _shared_ctx(S, vals, w, Vt, head)
    cut = twosd.build_sasa_cut(epi, SC.X[0], V, tie_rel=0.0, keep_picks=True)
    picks = twosd.picks_get(ctx, cut.picks)
    r, T, c0 = _template_arrays(ctx)
    M, seed, off = 33, 20240229, 1000
    R = twosd.reform_cuts(epi, [cut.picks], M, seed, index_offset=off)
    cnt = BR.counts(seed, off, N, M)
    dv = vals - S.tmpl
    for row in range(M + 1):
        c = None if row == 0 else cnt[:, row - 1].astype(np.float64)
        a, b, wm = BR.reform(r, T, c0, ctx.rows, ctx.cols, np.asarray(Vt), dv, w, picks, c)
        _close(R.alpha[row, 0], a, f"c-shared row {row} alpha")
        _close(R.beta[row, 0], b, f"c-shared row {row} beta")
        _close(R.weight_mark[row, 0], wm, f"c-shared row {row} weight_mark")
    _close(R.alpha[0, 0], cut.alpha, "c-shared identity alpha")
    _close(R.beta[0, 0], cut.beta, "c-shared identity beta")


# ---- 3. sampler and stream moments --------------------------------------------------------------------------
def _mixed_sto(S):
    """The three kinds over the RHS and T positions of the variant's listing (the construction of
    tests/test_gpu_sampler.py's _mixed_sto); the T positions include the structural zero of T."""
    from tests.test_gpu_sampler import _mixed_sto as base
    return base(S)


@pytest.mark.parametrize("tid", ["c", "e"])
def test_sampler_and_moments_with_T_positions(tid):
    from oracle import cpu
    from sqlp_amd import twosd
    S, vals, _, _, _ = _ref(tid, "distinct")
    sto = _mixed_sto(S)
    ctx = twosd.SDContext(S.sp2, sto, positions=S.positions)
    ctx.set_distributions(sto)
    ctx.compute_basis(SC.X[0], vals[0])
    dists = VR.dists_of(sto, ctx.positions)
    kinds = np.array([d[0] for d in dists])
    tpos = S.cols >= 0
    assert set(kinds[tpos]) | set(kinds[~tpos]) == {"DISCRETE", "NORMAL", "UNIFORM"} and (S.tmpl[tpos] == 0.0).any()
    exact = kinds != "NORMAL"
    seed, first = 0x9E3779B97F4A7C15, 2 ** 32 - 304

    def draw(n, sampling, first_index):
        epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
        twosd.add_sampled_scenarios(epi, n, seed, first_index=first_index, sampling=sampling)
        return twosd.get_scenarios(epi)

    n = 1000
    got = draw(n, None, first)                                                     # i.i.d., the counter carries inside
    ref = cpu.sample_deltas(sto, ctx.positions, ctx.template_values, n, seed, first) + ctx.template_values
    np.testing.assert_array_equal(got[:, exact], ref[:, exact])
    np.testing.assert_allclose(got[:, ~exact], ref[:, ~exact], rtol=1e-12, atol=1e-12)
    for plan, vr in ((twosd.Sampling.antithetic(), VR.antithetic(dists, 1024, seed, first)),
                     (twosd.Sampling.lhs(16), VR.lhs(dists, 16, 1024, seed, first))):
        g = draw(1024, plan, first)
        r = (vr - ctx.template_values) + ctx.template_values
        np.testing.assert_array_equal(g[:, exact], r[:, exact])
        for e in np.nonzero(~exact)[0]:
            mean, sd = dists[e][1], np.sqrt(dists[e][2])
            zg, zr = (g[:, e] - mean) / sd, (r[:, e] - mean) / sd
            assert (np.abs(zg - zr) / np.maximum(1.0, np.abs(zr))).max() <= 1e-12
    # the stream moments at X_Z against the oracle's objectives on the same stream
    from tests.test_gpu_evaluate_ci import _check_vs_oracle
    n = 2000
    m = twosd.evaluate_moments(ctx, np.zeros(len(S.xz)), S.xz, seed, 0, n)
    deltas = cpu.sample_deltas(sto, ctx.positions, ctx.template_values, n, seed)
    lp = _oracle_lp(S, ctx)
    o_obj, _, _, o_st, _ = lp.solve_batch(S.rows, S.r - S.T @ S.xz, deltas * SC.t_coef(S, S.xz)[None, :], nthreads=4)
    assert (o_st == 0).all()
    _check_vs_oracle(m, o_obj, f"{S.id} at X_Z")


# ---- 4. a position listed twice -------------------------------------------------------------------------------
def test_duplicate_position_refused():
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError, check, ptr
    S, vals, _, _, _ = _ref("c", "shared")
    ctx = _ctx(S, vals)
    t_e = int(np.nonzero(S.cols >= 0)[0][0])
    r_e = int(np.nonzero(S.cols < 0)[0][0])
    for dup in (t_e, r_e):                                  # the same (row, col) twice; two RHS entries of one row
        rows = np.ascontiguousarray(list(S.rows) + [S.rows[dup]], dtype=np.int32)
        cols = np.ascontiguousarray(list(S.cols) + [S.cols[dup]], dtype=np.int32)
        with pytest.raises(TwoSDError) as ei:
            check(ctx.lib.twosd_set_random_positions(ctx.h, len(rows), ptr(rows), ptr(cols), 0))
        assert ei.value.code == -1 and f"positions {dup} and {S.k}" in str(ei.value), str(ei.value)
        with pytest.raises(ValueError) as ev:
            ctx.set_positions(list(S.positions) + [S.positions[dup]])
        assert f"positions {dup} and {S.k}" in str(ev.value)
        assert ctx.k == S.k and [tuple(p) for p in ctx.positions] == S.positions
    with pytest.raises(ValueError):
        twosd.SDContext(S.sp2, positions=[S.positions[0], S.positions[1], S.positions[0]])
    # k and the positions are as they were: the solve is that of an untouched context
    obj, _, pi, st = ctx.solve_values(SC.X[1], vals, want_pi=True)
    other = _ctx(S, vals)
    obj2, _, pi2, st2 = other.solve_values(SC.X[1], vals, want_pi=True)
    assert (st == 0).all()
    np.testing.assert_array_equal(obj, obj2)
    np.testing.assert_array_equal(pi, pi2)
