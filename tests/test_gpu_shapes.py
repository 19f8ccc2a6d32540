"""Shape sweep: every instantiation of the LP kernel (lp_hyper_kernel<R, C, FULL>, R rows per
lane, C column slots per lane) and of the cut's argmax kernels (KB blocks of four k-rows), at
both edges of its slot, on the generated templates of tests/synth_cases.py, with the helpers
around them (dual vertex set, keyed push, pool build / refresh / selection) at those shapes, and
the envelope refusals.  The references are the C oracle and HiGHS; the assertions and tolerances
are those the suite applies to the SMPS instances (tests/test_gpu_lp.py, test_gpu_cut.py,
test_gpu_pool_refresh.py, test_gpu_bounds.py).  tests/test_synth_cases.py proves, without a GPU,
that the inputs have what these checks need."""
import os
import re

import numpy as np
import pytest

from tests import bounds_cases as BC
from tests import synth_cases as SC

pytestmark = pytest.mark.gpu

N = SC.N_SCEN


class _env:
    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        self.old = os.environ.get(self.key)
        os.environ[self.key] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop(self.key, None)
        else:
            os.environ[self.key] = self.old


def _ctx(S):
    """A context with the optimal basis of scenario 0 at X[0] as the primary basis: from the host
    setup solve, or from the committed head where that solve takes too long (synth_cases)."""
    from sqlp_amd import twosd
    ctx = twosd.SDContext(S.sp2, positions=S.positions)
    assert (ctx.m_lp, ctx.n_lp, ctx.k) == (S.m2, S.n2, S.k)
    if S.id in SC.GOLDEN_HEADS:
        ctx.set_basis(SC.golden_head(S.id))
    else:
        ctx.compute_basis(SC.X[0], SC.values(S)[0])
    return ctx


def _oracle(S, ctx, x, vals):
    from oracle import cpu
    lp = cpu.CpuLP(S.W, S.q, S.sense)
    lp.set_basis(ctx.get_basis())
    return lp.solve_batch(S.rows, S.r - S.T @ x, vals - S.r[S.rows], want_y=True, nthreads=4)


def _dual_feasible(S, pi, tol=1e-7):
    """tests/test_gpu_lp.py's _dual_feasible on every row of pi."""
    scale = 1.0 + np.abs(S.q).max()
    ok = (S.q[None, :] - pi @ S.W).min(1) >= -tol * scale
    for i, s in enumerate(S.sense):
        if s == "G":
            ok &= pi[:, i] >= -tol * scale
        elif s == "L":
            ok &= pi[:, i] <= tol * scale
    return ok


# ---- 1. LP: full and lean kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("tid", SC.MAIN_IDS)
def test_lp_matches_oracle_and_highs(tid):
    from oracle import lp_highs
    S = SC.template(tid)
    ctx = _ctx(S)
    x, vals = SC.X[0], SC.values(S)
    obj, y, pi, st = ctx.solve_values(x, vals, want_pi=True, want_y=True)
    assert (st == 0).all(), np.bincount(st)
    o_obj, o_pi, o_y, o_st, o_it = _oracle(S, ctx, x, vals)
    assert (o_st == 0).all()
    err = np.abs(obj - o_obj) / (1 + np.abs(o_obj))
    print(f"SHAPES lp {tid} (R, C, KB) = {S.dispatch}: worst objective error {err.max():.3e} relative, "
          f"oracle pivots mean {o_it.mean():.1f} max {o_it.max()}")
    np.testing.assert_allclose(obj, o_obj, rtol=1e-9, atol=1e-9)
    B = SC.rhs(S, x, vals)
    assert (np.abs(np.einsum("ij,ij->i", pi, B) - obj) <= 1e-9 * (1 + np.abs(obj))).all()      # strong duality
    assert _dual_feasible(S, pi).all()
    res = y @ S.W.T - B                                                                        # primal feasibility
    tolb = 1e-7 * (1 + np.abs(B))
    for i, s in enumerate(S.sense):
        if s == "G":
            assert (res[:, i] >= -tolb[:, i]).all()
        elif s == "L":
            assert (res[:, i] <= tolb[:, i]).all()
        else:
            assert (np.abs(res[:, i]) <= tolb[:, i]).all()
    assert (y >= -1e-9).all()
    for s in range(0, N, N // 16):
        hst, hobj, _, _ = lp_highs.solve_rhs(S.hp, B[s])
        assert hst == 0 and abs(hobj - obj[s]) <= 1e-8 * (1 + abs(hobj)), (s, hobj, obj[s])
    lean, _, _, st2 = ctx.solve_values(x, vals, want_pi=False)                                 # the lean kernel
    assert (st2 == 0).all()
    np.testing.assert_array_equal(lean, obj)
    # the dual is the oracle's wherever it is uniquely determined: every such scenario, no share cap
    unique = SC.unique_dual_mask(S, o_y, B)
    assert unique.mean() >= 0.9
    np.testing.assert_allclose(pi[unique], o_pi[unique], rtol=1e-9, atol=1e-9)


# ---- 2. pool build, refresh and selection -------------------------------------------------------------
def _pool_run(S, capfd):
    """pool_build at X[0], pool_refresh at X[1], solve there -> (P, heads, objectives, statuses,
    pivots, whether the device pool build ran)."""
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    ctx = _ctx(S)
    tr = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(tr, SC.values(S, SC.N_TRAIN, SC.SEED_TRAIN))
    if 520 * (S.k + 1) + 17 * 1024 > 160 * 1024:          # pool_build's LDS guard (pool_select_lds_bytes)
        with pytest.raises(TwoSDError) as ei:
            ctx.pool_build(tr, SC.X[0], 0, SC.N_TRAIN, 16)
        assert ei.value.code == -5 and "too many for pool selection" in str(ei.value)
        return None
    size = ctx.pool_build(tr, SC.X[0], 0, SC.N_TRAIN, 16)
    assert 1 <= size <= 16
    ev = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(ev, SC.values(S))
    capfd.readouterr()
    with _env("TWOSD_DEBUG", "1"):
        P = ctx.pool_refresh(tr, SC.X[1], 0, SC.N_TRAIN, 64)
    log = capfd.readouterr().err
    assert 1 <= P <= 64
    o, _, _, st = twosd.solve_batch(ev, SC.X[1], 0, N, want_pi=False)
    return P, [ctx.pool_get(p) for p in range(P)], o, st, ctx.lp_stats()[0], "pg_compute:" in log, log


@pytest.mark.parametrize("tid", SC.MAIN_IDS)
def test_pool_refresh_and_selection(tid, monkeypatch, capfd):
    S = SC.template(tid)
    runs = {}
    for mode in ("host", "device"):
        if mode == "host":
            monkeypatch.setenv("TWOSD_REFRESH_HOST", "1")
        else:
            monkeypatch.delenv("TWOSD_REFRESH_HOST", raising=False)
        runs[mode] = _pool_run(S, capfd)
    ref = _ctx(S)                                          # primary basis only
    o_ref, _, _, st_ref = ref.solve_values(SC.X[1], SC.values(S), want_pi=False)
    assert (st_ref == 0).all()
    if runs["device"] is None:                             # pool_build refused: the primary basis it is
        assert runs["host"] is None
        return
    (P_h, heads_h, o_h, st_h, piv_h, dev_h, _), (P_d, heads_d, o_d, st_d, piv_d, dev_d, log) = runs["host"], runs["device"]
    assert (st_h == 0).all() and (st_d == 0).all()
    np.testing.assert_allclose(o_d, o_ref, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(o_h, o_ref, rtol=1e-9, atol=1e-9)
    assert P_h == P_d
    for a, b in zip(heads_h, heads_d):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_allclose(o_d, o_h, rtol=1e-12, atol=1e-12)
    assert piv_d == piv_h
    assert not dev_h
    # the device build runs wherever its LDS layouts fit and a basis was picked; past that the
    # refresh composes on the host (the limits): no device build in the log, same pool
    picked = int(re.search(r"\(R=(\d+)\)", log).group(1))
    assert dev_d == (picked > 0 and SC.pg_supported(S.m2, S.n2)), log
    # every picked basis is kept, on the device and on the host path: none is lost to a full eta
    # arena (the refresh solves again with a larger one) and none fails the checks
    assert P_d == picked + 1, (P_d, picked)
    if tid != "a":
        assert P_d > 1
    print(f"SHAPES pool {tid}: picked {picked}, pool {P_d}, device build {dev_d}, pivots {piv_d / N:.2f} a scenario")


def test_refresh_solves_again_when_the_eta_arena_is_full(monkeypatch, capfd):
    """Template n refreshed at X_FAR: 512 training solves of about 33 pivots on 600 rows, whose eta
    files do not fit the first arena of 4096 entries per scenario.  Files that do not fit are lost in
    the order the waves finish, so the pool used to differ from run to run (22 to 25 of 64 bases
    kept).  The refresh now solves again with an arena of the size asked for: no file is lost,
    and the host and device builds give the same pool, pivots and objectives."""
    S = SC.template("n")
    monkeypatch.setattr(SC, "X", [SC.X[0], SC.X_FAR])
    runs = {}
    for mode in ("host", "device"):
        if mode == "host":
            monkeypatch.setenv("TWOSD_REFRESH_HOST", "1")
        else:
            monkeypatch.delenv("TWOSD_REFRESH_HOST", raising=False)
        runs[mode] = _pool_run(S, capfd)
    (P_h, heads_h, o_h, st_h, piv_h, _, log_h), (P_d, heads_d, o_d, st_d, piv_d, dev_d, log_d) = runs["host"], runs["device"]
    assert "solved again" in log_h and "solved again" in log_d and dev_d
    picked = int(re.search(r"\(R=(\d+)\)", log_d).group(1))
    print(f"SHAPES arena n at X_FAR: picked {picked}, pool {P_d}")
    assert P_h == P_d == picked + 1                       # a full arena left 22 to 25 of them
    for a, b in zip(heads_h, heads_d):
        np.testing.assert_array_equal(a, b)
    assert (st_h == 0).all() and (st_d == 0).all() and piv_d == piv_h
    np.testing.assert_allclose(o_d, o_h, rtol=1e-12, atol=1e-12)
    ref = _ctx(S)
    o_ref, _, _, st_ref = ref.solve_values(SC.X_FAR, SC.values(S), want_pi=False)
    assert (st_ref == 0).all()
    np.testing.assert_allclose(o_d, o_ref, rtol=1e-9, atol=1e-9)


# ---- 3. dual vertex set and keyed push ----------------------------------------------------------------
def _push_run(S):
    from sqlp_amd import twosd
    ctx = _ctx(S)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, SC.values(S))
    obj, st, nv = twosd.solve_push(epi, SC.X[0], 0, N)
    assert (st == 0).all()
    Vm = twosd.sdDualVertexSet(ctx).matrix()
    assert nv == len(Vm)
    return obj, Vm


@pytest.mark.parametrize("tid", SC.MAIN_IDS + SC.KB_IDS)
def test_dual_vertex_set_and_keyed_push(tid):
    from oracle import twosd_ref
    from sqlp_amd import twosd
    S = SC.template(tid)
    ctx = _ctx(S)
    _, _, pi, st = ctx.solve_values(SC.X[0], SC.values(S), want_pi=True)
    assert (st == 0).all()
    V = twosd.sdDualVertexSet(ctx)
    ref = twosd_ref.DualVertexSet()
    for blk in np.array_split(pi, [1, 50, 51, 220]):
        assert V.push_batch(blk).tolist() == ref.push_batch(blk).tolist()
    assert len(V) == len(ref) and (tid == "a" or len(V) >= 30)
    np.testing.assert_array_equal(V.matrix(), ref.matrix(S.m2))
    obj, Vm = _push_run(S)                                 # keyed
    with _env("TWOSD_PUSH_ALL", "1"):
        obj2, Vm2 = _push_run(S)
    assert np.array_equal(obj, obj2) and np.array_equal(Vm, Vm2)


# ---- 4. cut -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tid", SC.MAIN_IDS + SC.KB_IDS)
def test_cut_matches_oracle(tid):
    from oracle import cpu
    from sqlp_amd import twosd
    S = SC.template(tid)
    ctx = _ctx(S)
    vals = SC.values(S)
    _, _, pi, st = ctx.solve_values(SC.X[0], vals, want_pi=True)
    assert (st == 0).all()
    V = twosd.sdDualVertexSet(ctx)
    V.push_batch(pi)
    Vm = V.matrix()
    w = SC.weights()
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals, w)
    p = w / w.sum()
    ra = np.tile(S.r, (N, 1))
    ra[:, S.rows] = vals
    worst = 0.0
    kinds = set()
    for x in SC.X:                                          # where V was built, and elsewhere
        scores = SC.cut_scores(S, Vm, x, vals)
        best = scores.max(1)
        for tie_rel in (0.0, 1e-12):
            a, b, omv, oma = cpu.build_cut(S.r, S.T, x, Vm, S.rows, vals - S.r[S.rows], w, tie_rel=tie_rel, nthreads=4)
            got = {}
            for kind in (2, 1, 0):                          # the integer, fp32 and fp64 passes requested
                f32, i8 = SC.PASS_ENV[kind]["TWOSD_CUT_F32"], SC.PASS_ENV[kind]["TWOSD_CUT_I8"]
                with _env("TWOSD_CUT_F32", f32), _env("TWOSD_CUT_I8", i8):
                    cut, mv, ma = twosd._build_cut(epi, x, tie_rel, want_argmax=True)
                    got[f32] = ctx.cut_pass()
                    ran = ctx.cut_pass_kind()[0]
                assert got[f32][0] == int(f32)
                # the fp64 and fp32 requests run those passes; the integer request runs the integer pass,
                # or the fp32 one where the integer band is not finite (recorded per template below)
                assert ran == kind or (kind == 2 and ran == 1), (kind, ran)
                kinds.add((kind, ran))
                assert cut.weight_mark == pytest.approx(w.sum(), rel=1e-15)
                assert (ma == oma).all(), (f32, tie_rel, SC.near_ties(scores), int((ma != oma).sum()))
                np.testing.assert_allclose(mv, omv, rtol=1e-10, atol=1e-9)
                assert (scores[np.arange(N), ma] >= best - 1e-9 * (1 + np.abs(best))).all()
                worst = max(worst, abs(cut.alpha - a) / (1 + abs(a)))
                assert cut.alpha == pytest.approx(a, rel=1e-8, abs=1e-8)
                np.testing.assert_allclose(cut.beta, b, rtol=1e-8, atol=1e-8 * (1 + np.abs(b).max()))
                # the reference formula (epigraph.jl:134-143) over the GPU's own choices
                a_ref = float(np.sum(p * np.einsum("ij,ij->i", Vm[ma], ra)))
                b_ref = -(S.T.T @ (p @ Vm[ma]))
                assert cut.alpha == pytest.approx(a_ref, rel=1e-9, abs=1e-9)
                np.testing.assert_allclose(cut.beta, b_ref, rtol=1e-9, atol=1e-9 * (1 + np.abs(b_ref).max()))
            assert got["1"][1] > got["0"][1] > 0.0         # the fp32 band is the wider one
    print(f"SHAPES cut {tid} (R, C, KB) = {S.dispatch}: |V| {len(Vm)}, worst alpha error {worst:.3e} relative, "
          f"passes run for the integer request {sorted(r for q, r in kinds if q == 2)}")


# ---- 5. envelope --------------------------------------------------------------------------------------
def _usable():
    """The library still serves a context after a refusal."""
    S = SC.template("c")
    ctx = _ctx(S)
    obj, _, _, st = ctx.solve_values(SC.X[0], SC.values(S)[:8], want_pi=False)
    assert (st == 0).all() and np.isfinite(obj).all()


def test_envelope_1025_rows_refused():
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    m2 = 1025
    big = BC.stage_problem(np.eye(m2), np.zeros((m2, 1)), np.ones(m2), np.ones(m2), ["E"] * m2, np.zeros(m2), np.full(m2, np.inf))
    with pytest.raises(TwoSDError) as ei:
        twosd.SDContext(big)
    assert ei.value.code == -5 and "1025 LP rows exceed the LP kernel envelope (1024 rows)" in str(ei.value)
    _usable()


def test_envelope_4097_columns_refused():
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    m2, n2 = 8, 4089
    W = np.zeros((m2, n2))
    W[np.arange(n2) % m2, np.arange(n2)] = 1.0
    wide = BC.stage_problem(W, np.zeros((m2, 1)), np.ones(n2), np.ones(m2), ["E"] * m2, np.zeros(n2), np.full(n2, np.inf))
    with pytest.raises(TwoSDError) as ei:
        twosd.SDContext(wide)
    assert ei.value.code == -5 and "4097 LP columns and rows exceed 4096 columns" in str(ei.value)
    ok = BC.stage_problem(W[:, :-1], np.zeros((m2, 1)), np.ones(n2 - 1), np.ones(m2), ["E"] * m2, np.zeros(n2 - 1),
                          np.full(n2 - 1, np.inf))
    ctx = twosd.SDContext(ok)                              # 4096 is inside
    assert ctx.n_lp + ctx.m_lp == 4096
    _usable()


def test_envelope_128_elements_refused_by_the_cut_only():
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    S = SC.synth_template(160, 400, 128, seed=228, amp=0.2)
    S.id = "k128"
    ctx = _ctx(S)
    vals = SC.values(S)
    obj, _, pi, st = ctx.solve_values(SC.X[0], vals, want_pi=True)
    assert (st == 0).all()
    o_obj, _, _, o_st, _ = _oracle(S, ctx, SC.X[0], vals)
    np.testing.assert_allclose(obj, o_obj, rtol=1e-9, atol=1e-9)
    V = twosd.sdDualVertexSet(ctx)
    V.push_batch(pi)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals)
    with pytest.raises(TwoSDError) as ei:
        twosd.build_sasa_cut(epi, SC.X[0], V)
    assert ei.value.code == -5 and "k = 128 random elements exceeds the cut kernel envelope (127)" in str(ei.value)
    obj2, _, _, st2 = twosd.solve_batch(epi, SC.X[0], 0, N, want_pi=False)      # the context still solves
    assert (st2 == 0).all()
    np.testing.assert_array_equal(obj2, obj)
