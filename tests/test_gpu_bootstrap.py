"""Stored picks, the Poisson(1) replicate counts and the bootstrap re-formation of cuts
(sqlp_amd/csrc/boot_kernel.hip) against the numpy restatement tests/boot_ref.py, and the stopping
rule end to end on lands.  The reference has no counterpart (plugin/stopping_rule.jl is empty).

Tolerance: the project's cut tolerance, 1e-8 relative to 1 + |reference| (tests/test_gpu_sd_loop.py).
Shapes: N = 300 (no multiple of the 64-scenario tile, several tiles and waves), N in {1, 63, 64, 65}
around one tile, k = 1 .. 120 (one and two elements per lane: the kernel's two instantiations),
M in {1, 33, 64} (one replicate, a group of 16 with one member, four full groups), and lands at
N = 2500: 40 tiles in 10 shards, more than the eight segments the shards' partials are summed in
(sqlp_amd/csrc/reform_layout.h, reform.hip)."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import boot_ref as BR
from tests import bounds_cases as BC
from tests import instances as I
from tests import synth_cases as SC

pytestmark = pytest.mark.gpu

SYNTH = ["a", "l", "k87", "k88", "k119", "k120"]
NAMES = ["lands", "transship", "randT", "boxed"] + SYNTH
STAGES = [(0, 100), (100, 200), (200, 300)]
SEED = 20240229


def _close(got, ref, what):
    """|got - ref| <= 1e-8 (1 + |ref|): per entry for scalars per cut (alpha, weights), against the
    largest entry of each cut's beta vector (the existing cut tests' rule for beta)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = np.abs(ref).max(axis=-1, keepdims=True) if "beta" in what and ref.ndim else np.abs(ref)
    ratio = np.abs(got - ref) / (1e-8 * (1.0 + scale))
    worst = ratio.max(initial=0.0)
    print(f"{what}: worst error {worst:.3e} of the bound")
    assert worst <= 1.0, (what, worst)


def _template_arrays(ctx):
    """(r, T, c0) of the LP the kernels solve: the caller's, or the canonical form's."""
    from sqlp_amd import twosd
    sp2 = ctx.sp2
    T = sp2.dense_T()
    cf = twosd.canonical_form(sp2.W, sp2.q, sp2.r, sp2.sense, sp2.ylb, sp2.yub)
    return np.asarray(cf.r), np.vstack([T, np.zeros((cf.m_lp - T.shape[0], T.shape[1]))]), cf.c0


def _context(name):
    """(ctx, x, [(values, weights) per epigraph]) of an instance, 300 scenarios per epigraph."""
    from sqlp_amd import smps, twosd
    rng = np.random.default_rng(7)
    if name in ("lands", "transship"):
        inst = I.load(name)
        ctx = twosd.SDContext(inst["sp2"], inst["sto"])
        x = I.x_ev(name)
        ctx.compute_basis(x, smps.mean_values(inst["sto"]))
        if name == "lands":
            return ctx, x, [(I.sample(name, 300, 3), np.ones(300))]
        return ctx, x, [(I.sample(name, 300, 3 + e), rng.uniform(0.5, 1.5, size=300)) for e in range(2)]
    if name == "randT":
        from tests import test_gpu_parity_paths as PP
        positions, vals = PP._t_scenarios("lands", 300, seed=31)
        ctx, x = PP._ctx("lands", positions=positions)
        return ctx, x, [(vals, rng.uniform(0.5, 1.5, size=300))]
    if name == "boxed":
        S = BC.slot_template()
        ctx = twosd.SDContext(S.sp2, positions=[("RHS", f"r{i}") for i in S.rows])
        assert ctx.n_bound_rows == 10
        vals = S.r[S.rows] + np.random.default_rng(0).uniform(-1.0, 1.0, size=(300, len(S.rows)))
        x = np.array([0.5, 1.0, 0.2, 0.7])
        ctx.compute_basis(x, vals[0])
        return ctx, x, [(vals, rng.uniform(0.5, 1.5, size=300))]
    S = SC.template(name)
    ctx = twosd.SDContext(S.sp2, positions=S.positions)
    ctx.compute_basis(SC.X[0], SC.values(S)[0])
    return ctx, SC.X[0], [(SC.values(S), SC.weights())]


_BUILT = {}


@pytest.fixture(scope="module", autouse=True)
def _close_shared_contexts():
    """The instances shared by this module's tests live until its last test, then return their
    device memory (later modules measure the free memory)."""
    yield
    for B in _BUILT.values():
        B.ctx.close()
    _BUILT.clear()
    BR.counts.cache_clear()
    import gc
    gc.collect()


def _built(name):
    if name not in _BUILT:
        _BUILT[name] = _build(name)
    return _BUILT[name]


def _build(name):
    """The instance with, per epigraph, three cuts kept at N_j = 100 / 200 / 300 scenarios, new
    vertices pushed before each (so nv_j grows and the first handles have nv below |V| and N_j < N)."""
    from sqlp_amd import twosd
    ctx, x, data = _context(name)
    r, T, c0 = _template_arrays(ctx)
    V = twosd.sdDualVertexSet(ctx)
    epis = []
    for vals, w in data:
        epi = twosd.sdEpigraph(ctx, 1.0 / len(data), 0.0)
        kept = []
        for j, (lo, hi) in enumerate(STAGES):
            twosd.add_scenarios(epi, vals[lo:hi], w[lo:hi])
            xs = x * (1.0 + 0.03 * j)
            twosd.solve_push(epi, xs, lo, hi - lo)
            cut, mv, ma = twosd._build_cut(epi, xs, 0.0, want_argmax=True)
            h = twosd.keep_picks_of_last_cut(epi)
            kept.append(SimpleNamespace(cut=cut, arg=ma.copy(), h=h, n=hi, nv=len(V)))
        epis.append(SimpleNamespace(epi=epi, kept=kept, dv=vals - ctx.template_values, w=w))
    return SimpleNamespace(ctx=ctx, x=x, r=r, T=T, c0=c0, V=V, epis=epis)


def _ref_rows(B, E, M, seed, off):
    """boot_ref's (alpha, beta, weight_mark, total_weight) in reform_cuts' layout."""
    ctx = B.ctx
    Vm = B.V.matrix()
    N = len(E.w)
    cnt = BR.counts(seed, off, N, M) if M else np.zeros((N, 0), dtype=np.uint8)
    H = len(E.kept)
    a = np.zeros((M + 1, H)); b = np.zeros((M + 1, H, ctx.n1)); wm = np.zeros((M + 1, H)); tw = np.zeros(M + 1)
    for row in range(M + 1):
        c = None if row == 0 else cnt[:, row - 1].astype(np.float64)
        tw[row] = float(np.sum((np.ones(N) if c is None else c) * E.w))
        for j, K in enumerate(E.kept):
            a[row, j], b[row, j], wm[row, j] = BR.reform(B.r, B.T, B.c0, ctx.rows, ctx.cols, Vm, E.dv, E.w, K.arg,
                                                         None if c is None else c[:K.n])
    return a, b, wm, tw


# ---------------------------------------------------------------- counts
@pytest.mark.parametrize("first", [0, 2 ** 32 - 3])
@pytest.mark.parametrize("M", [1, 4, 5, 64])
def test_counts_bit_equal(M, first):
    from sqlp_amd import twosd
    ctx = _built("lands").ctx
    got = twosd.bootstrap_counts(ctx, M, SEED, first, 300)
    np.testing.assert_array_equal(got, BR.counts(SEED, first, 300, M))
    assert got.max() <= 12
    # a range drawn in two pieces equals one draw
    two = np.vstack([twosd.bootstrap_counts(ctx, M, SEED, first, 117), twosd.bootstrap_counts(ctx, M, SEED, first + 117, 183)])
    np.testing.assert_array_equal(two, got)


# ---------------------------------------------------------------- identity row and replicates
@pytest.mark.parametrize("name", NAMES)
def test_identity_row_is_the_cut(name):
    from sqlp_amd import twosd
    B = _built(name)
    for E in B.epis:
        R = twosd.reform_cuts(E.epi, [K.h for K in E.kept], 0, SEED)
        assert R.alpha.shape == (1, 3) and R.beta.shape == (1, 3, B.ctx.n1)
        for j, K in enumerate(E.kept):
            assert twosd.picks_info(B.ctx, K.h) == (E.epi.index, K.n, K.nv)
            np.testing.assert_array_equal(twosd.picks_get(B.ctx, K.h), K.arg)
            _close(R.alpha[0, j], K.cut.alpha, f"{name} alpha[{j}]")
            _close(R.beta[0, j], K.cut.beta, f"{name} beta[{j}]")
            _close(R.weight_mark[0, j], K.cut.weight_mark, f"{name} weight_mark[{j}]")
        _close(R.total_weight[0], E.epi.total_scenario_weight, f"{name} total weight")


@pytest.mark.parametrize("M,off", [(1, 0), (33, 1000), (64, 0)])
@pytest.mark.parametrize("name", NAMES)
def test_replicates_match_restatement(name, M, off):
    from sqlp_amd import twosd
    B = _built(name)
    for e, E in enumerate(B.epis):
        R = twosd.reform_cuts(E.epi, [K.h for K in E.kept], M, SEED + e, index_offset=off)
        a, b, wm, tw = _ref_rows(B, E, M, SEED + e, off)
        _close(R.alpha, a, f"{name} M={M} alpha")
        _close(R.beta, b, f"{name} M={M} beta")
        _close(R.weight_mark, wm, f"{name} M={M} weight_mark")
        _close(R.total_weight, tw, f"{name} M={M} total_weight")


@pytest.mark.parametrize("N", [1, 63, 64, 65])
@pytest.mark.parametrize("name", NAMES)
def test_replicates_around_one_tile(name, N):
    """One handle over N scenarios (a partial tile, exactly one, one and a row), every M."""
    from sqlp_amd import twosd
    ctx, x, data = _context(name)
    vals, w = data[0][0][:N], np.random.default_rng(9).uniform(0.5, 1.5, size=N)
    r, T, c0 = _template_arrays(ctx)
    V = twosd.sdDualVertexSet(ctx)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals, w)
    twosd.solve_push(epi, x, 0, N)
    cut, _, ma = twosd._build_cut(epi, x, 0.0, want_argmax=True)
    h = twosd.keep_picks_of_last_cut(epi)
    B = SimpleNamespace(ctx=ctx, r=r, T=T, c0=c0, V=V)
    E = SimpleNamespace(w=w, dv=vals - ctx.template_values, kept=[SimpleNamespace(arg=ma, n=N)])
    for M, off in [(1, 1000), (33, 0), (64, 1000)]:
        R = twosd.reform_cuts(epi, [h], M, SEED, index_offset=off)
        a, b, wm, tw = _ref_rows(B, E, M, SEED, off)
        _close(R.alpha, a, f"{name} N={N} M={M} alpha")
        _close(R.beta, b, f"{name} N={N} M={M} beta")
        _close(R.weight_mark, wm, f"{name} N={N} M={M} weight_mark")
        _close(R.total_weight, tw, f"{name} N={N} M={M} total_weight")
    _close(R.alpha[0, 0], cut.alpha, "identity alpha")
    ctx.close()


def test_replicates_past_eight_shards():
    """One handle over 2500 scenarios: 10 shards, so some of the eight segments add two."""
    from sqlp_amd import twosd
    N, M = 2500, 1
    ctx, x, _ = _context("lands")
    vals, w = I.sample("lands", N, 3), np.random.default_rng(9).uniform(0.5, 1.5, size=N)
    r, T, c0 = _template_arrays(ctx)
    V = twosd.sdDualVertexSet(ctx)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals, w)
    twosd.solve_push(epi, x, 0, N)
    cut, _, ma = twosd._build_cut(epi, x, 0.0, want_argmax=True)
    h = twosd.keep_picks_of_last_cut(epi)
    B = SimpleNamespace(ctx=ctx, r=r, T=T, c0=c0, V=V)
    E = SimpleNamespace(w=w, dv=vals - ctx.template_values, kept=[SimpleNamespace(arg=ma, n=N)])
    R = twosd.reform_cuts(epi, [h], M, SEED)
    a, b, wm, tw = _ref_rows(B, E, M, SEED, 0)
    _close(R.alpha, a, f"lands N={N} M={M} alpha")
    _close(R.beta, b, f"lands N={N} M={M} beta")
    _close(R.weight_mark, wm, f"lands N={N} M={M} weight_mark")
    _close(R.total_weight, tw, f"lands N={N} M={M} total_weight")
    _close(R.alpha[0, 0], cut.alpha, "identity alpha")
    ctx.close()


def test_zero_weight_replicate_gives_the_zero_cut():
    from sqlp_amd import twosd
    seed = next(s for s in range(1000) if (lambda c: (c == 0).any() and (c >= 2).any())(BR.counts(s, 0, 1, 64)[0]))
    ctx, x, data = _context("lands")
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, data[0][0][:1], np.array([1.5]))
    twosd.solve_push(epi, x, 0, 1)
    cut = twosd.build_sasa_cut(epi, x, twosd.sdDualVertexSet(ctx), keep_picks=True)
    R = twosd.reform_cuts(epi, [cut], 64, seed)
    c = BR.counts(seed, 0, 1, 64)[0].astype(np.float64)
    zero = np.flatnonzero(c == 0) + 1
    assert len(zero) >= 1
    assert (R.alpha[zero] == 0.0).all() and (R.beta[zero] == 0.0).all() and (R.weight_mark[zero] == 0.0).all()
    assert (R.total_weight[zero] == 0.0).all()
    live = np.flatnonzero(c > 0) + 1
    _close(R.weight_mark[live, 0], 1.5 * c[live - 1], "weight_mark = count * weight")
    _close(R.alpha[live, 0], np.full(len(live), cut.alpha), "one scenario: every live replicate is the cut")
    ctx.close()


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("name", ["transship", "k119"])
def test_same_bits_every_call_and_per_handle(name):
    from sqlp_amd import twosd
    B = _built(name)
    E = B.epis[-1]
    hs = [K.h for K in E.kept]
    R1 = twosd.reform_cuts(E.epi, hs, 33, SEED, index_offset=5)
    R2 = twosd.reform_cuts(E.epi, hs, 33, SEED, index_offset=5)
    for f in ("alpha", "beta", "weight_mark", "total_weight"):
        np.testing.assert_array_equal(getattr(R1, f), getattr(R2, f))
    for j, h in enumerate(hs):
        Rj = twosd.reform_cuts(E.epi, [h], 33, SEED, index_offset=5)
        np.testing.assert_array_equal(Rj.alpha[:, 0], R1.alpha[:, j])
        np.testing.assert_array_equal(Rj.beta[:, 0], R1.beta[:, j])
        np.testing.assert_array_equal(Rj.weight_mark[:, 0], R1.weight_mark[:, j])
        np.testing.assert_array_equal(Rj.total_weight, R1.total_weight)


# ---------------------------------------------------------------- the two-rank split
def test_split_over_two_contexts():
    import torch
    from sqlp_amd import twosd
    M, N, half = 33, 300, 150
    ctx, x, data = _context("transship")
    vals, w = data[0]
    V = twosd.sdDualVertexSet(ctx)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals, w)
    twosd.solve_push(epi, x, 0, N)
    _, _, ma = twosd._build_cut(epi, x, 0.0, want_argmax=True)
    h = twosd.keep_picks_of_last_cut(epi)
    total = epi.total_scenario_weight
    whole = twosd.reform_cuts(epi, [h], M, SEED)
    nu, nf = twosd.reform_partial_len(ctx, [h], M)

    def bufs():
        return torch.zeros(nu, dtype=torch.int64, device="cuda"), torch.zeros(nf, dtype=torch.float64, device="cuda")
    u0, f0 = bufs()
    twosd.reform_partial(epi, [h], M, SEED, 0, total, u0.data_ptr(), f0.data_ptr())
    ranks = []
    for rk in range(2):
        c2, _, _ = _context("transship")
        V2 = twosd.sdDualVertexSet(c2)
        V2.push_batch(V.matrix())
        assert V2.fingerprint() == V.fingerprint()
        e2 = twosd.sdEpigraph(c2, 1.0, 0.0)
        sl = slice(rk * half, (rk + 1) * half)
        twosd.add_scenarios(e2, vals[sl], w[sl])
        _, _, ma2 = twosd._build_cut(e2, x, 0.0, want_argmax=True)
        np.testing.assert_array_equal(ma2, ma[sl])
        h2 = twosd.keep_picks_of_last_cut(e2)
        assert twosd.reform_partial_len(c2, [h2], M) == (nu, nf)
        u, f = bufs()
        twosd.reform_partial(e2, [h2], M, SEED, rk * half, total, u.data_ptr(), f.data_ptr())
        ranks.append((c2, h2, u, f))
    u = ranks[0][2] + ranks[1][2]      # rank order
    f = ranks[0][3] + ranks[1][3]
    torch.cuda.synchronize()
    # the totals, the W_jb and the per-vertex weights are integers: exact under the split
    assert torch.equal(u, u0)
    for c2, h2, _, _ in ranks:
        R = twosd.reform_finalize(c2, [h2], M, total, u.data_ptr(), f.data_ptr())
        np.testing.assert_array_equal(R.weight_mark, whole.weight_mark)
        np.testing.assert_array_equal(R.total_weight, whole.total_weight)
        _close(R.alpha, whole.alpha, "split alpha")
        _close(R.beta, whole.beta, "split beta")
    for c2, _, _, _ in ranks:
        c2.close()
    ctx.close()


# ---------------------------------------------------------------- refusals
def test_refusals():
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    inst = I.load("lands")
    ctx, x, data = _context("lands")
    vals = data[0][0]
    V = twosd.sdDualVertexSet(ctx)
    ea, eb = twosd.sdEpigraph(ctx, 0.5, 0.0), twosd.sdEpigraph(ctx, 0.5, 0.0)
    twosd.add_scenarios(ea, vals[:40])
    twosd.add_scenarios(eb, vals[40:80])
    twosd.solve_push(ea, x, 0, 40)
    nv0 = len(V)
    ca = twosd.build_sasa_cut(ea, x, V, keep_picks=True)
    twosd.solve_push(eb, 1.2 * x, 0, 40)
    cb = twosd.build_sasa_cut(eb, 1.2 * x, V, keep_picks=True)
    assert twosd.picks_count(ctx) == 2 and twosd.picks_info(ctx, ca.picks)[2] == nv0

    def refused(code, text, f, *args, **kw):
        with pytest.raises(TwoSDError) as ei:
            f(*args, **kw)
        assert ei.value.code == code and text in str(ei.value), str(ei.value)
    refused(-1, "pick handle 99 does not exist", twosd.reform_cuts, ea, [99], 4, SEED)
    refused(-1, f"belongs to epigraph {eb.index}, not {ea.index}", twosd.reform_cuts, ea, [ca, cb], 4, SEED)
    refused(-1, "M = 65 replicates outside [0, 64]", twosd.reform_cuts, ea, [ca], 65, SEED)
    refused(-3, f"the last cut was built on epigraph {eb.index}, not {ea.index}", twosd.keep_picks_of_last_cut, ea)
    # an empty epigraph's cut has no picks to keep
    ec = twosd.sdEpigraph(ctx, 0.0, 0.0)
    assert twosd.build_sasa_cut(ec, x, V, keep_picks=True).picks is None
    refused(-3, "empty-epigraph path", twosd.keep_picks_of_last_cut, ec)
    # truncation below a handle's nv: cb (built over more vertices) dies, ca lives when nv0 stays
    assert len(V) > nv0
    V.truncate(nv0)
    refused(-3, "truncated", twosd.reform_cuts, eb, [cb], 4, SEED)
    refused(-3, "truncated", twosd.picks_get, ctx, cb.picks)
    assert twosd.reform_cuts(ea, [ca], 4, SEED).alpha.shape == (5, 1)
    refused(-3, "no cut to keep", twosd.keep_picks_of_last_cut, eb)      # the vertex set was reset since
    twosd.picks_release(ctx, cb.picks)
    refused(-1, "does not exist", twosd.picks_release, ctx, cb.picks)
    # a new template drops every handle
    ctx._set_problem(inst["sp2"], inst["sto"])
    assert twosd.picks_count(ctx) == 0
    refused(-1, "does not exist", twosd.picks_info, ctx, ca.picks)
    refused(-1, "does not exist", twosd.reform_cuts, ea, [ca], 4, SEED)
    ctx.close()


# ---------------------------------------------------------------- end to end
def _run_lands(seed):
    from sqlp_amd import master, stopping, twosd
    from tests.test_gpu_sd_loop import _lands_cell
    cell, sp1, sp2 = _lands_cell()
    rng = np.random.default_rng(42)
    tests = []

    def stop(c):
        res = stopping.bootstrap_gap_test(c, M=16, seed=seed)
        epi_r, alpha, beta, _ = c.cuts.rows()
        np.testing.assert_array_equal(res.rows0[0], epi_r)
        _close(res.rows0[1], alpha, "row-0 master alpha")
        _close(res.rows0[2], beta, "row-0 master beta")
        assert res.gaps[0] >= -1e-8 * (1 + abs(res.U[0])), res.gaps[0]
        assert twosd.picks_count(c.ctx) == len(c.epi[0].cuts) + 1      # the cuts held and the incumbent cut: no leak
        tests.append(res)
        return SimpleNamespace(passed=False, res=res)
    it, last = master.sd_run(cell, lambda i: [np.array([rng.choice([3.0, 5.0, 7.0], p=[0.3, 0.4, 0.3])])], 30, check_every=10,
                             stop=stop, quad_scalar_schedule=master.ConstantQuadScalarSchedule(0.1))
    assert it == 30 and len(tests) == 3 and last.res is tests[-1]
    cell.ctx.close()
    return tests


def test_sd_run_lands_end_to_end():
    a, b = _run_lands(5), _run_lands(5)
    for ra, rb in zip(a, b):
        np.testing.assert_array_equal(ra.U, rb.U)
        np.testing.assert_array_equal(ra.L, rb.L)
        assert ra.fraction == rb.fraction and ra.passed == rb.passed
    print("lands gaps at 10/20/30:", [float(r.gaps[0]) for r in a], "fractions", [r.fraction for r in a])


def test_gap_test_needs_picks():
    from sqlp_amd import master, stopping
    from tests.test_gpu_sd_loop import _lands_cell
    cell, _, _ = _lands_cell()
    master.sd_iteration(cell, [np.array([5.0])])
    with pytest.raises(ValueError, match="carries no picks"):
        stopping.bootstrap_gap_test(cell)
    cell.ctx.close()
