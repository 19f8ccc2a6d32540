"""The cut's integer (int8-limb) MFMA pass on the GPU: its score terms against the numpy model
bit for bit, its picks against the fp32 and fp64 passes and the C oracle, the tail ranges, the
fallbacks and the split cut."""
import os

import numpy as np
import pytest

from tests import cut_i8_model as M
from tests import instances as I
from tests import synth_cases as SC

pytestmark = pytest.mark.gpu


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


PASS_ENV = SC.PASS_ENV


# ---- bit-exact scores ---------------------------------------------------------------------------------
def _synth(k):
    S = SC.synth_template(160, 400, k, seed=900 + k, amp=0.2)
    S.id = f"i8k{k}"
    return S


@pytest.mark.parametrize("k", [1, 63, 64, 65, 117, 127])
def test_scores_equal_the_numpy_model_bit_for_bit(k):
    """twosd_cut_debug_scores == the model for N in {1, 127, 129, 300} x |V| in {1, 31, 33, 70}: both
    k-step instantiations, partial k-steps, partial tiles and partial chunks.  Vertices and deltas
    span six decades per row; with k > 1 one element has no variation (dmax_e = 0)."""
    from sqlp_amd import twosd
    S = _synth(k)
    ctx = twosd.SDContext(S.sp2, positions=S.positions)
    rng = np.random.default_rng(k)
    Vsrc = rng.normal(size=(70, S.m2)) * 10.0 ** rng.uniform(-3, 3, size=(70, S.m2)) * 10.0 ** rng.uniform(-2, 2, size=(70, 1))
    V = twosd.sdDualVertexSet(ctx)
    V.push_batch(Vsrc)
    assert len(V) == 70
    x = SC.X[0]
    dvs = {}
    for N in (1, 127, 129, 300):
        dv = rng.normal(size=(N, k)) * 10.0 ** rng.uniform(-3, 3, size=(1, k)) * 10.0 ** rng.uniform(-2, 0, size=(N, k))
        if k > 1:
            dv[:, k // 2] = 0.0
        vals = S.r[S.rows] + dv
        epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
        twosd.add_scenarios(epi, vals)
        dvs[N] = (epi, vals - S.r[S.rows])
    for nv in (70, 33, 31, 1):
        V.truncate(nv)
        Vm = V.matrix()
        for N, (epi, dv) in dvs.items():
            t, vmap = ctx.cut_debug_scores(epi.index, x, N, nv)
            kind, L, pairs = ctx.cut_pass_kind()
            assert kind == 2 and pairs == L * (L + 1) // 2
            assert t.shape == (N, len(vmap)) and len(vmap) == nv          # random rows: no twins
            pc = Vm[vmap][:, S.rows]                                        # RHS elements: coef = 1
            want = M.scores(pc, dv, np.abs(dv).max(axis=0), L)
            assert np.array_equal(t.view(np.uint32), want.view(np.uint32)), (k, N, nv, float(np.abs(t - want).max()))
            # and the term is within the band term of the exact dot product
            exact = dv @ pc.T
            assert (np.abs(t.astype(np.float64) - exact) <= M.vertex_band(pc, np.abs(dv).max(axis=0), L)[None, :] + 1e-12 * np.abs(exact)).all()


def test_k_128_is_refused_as_before():
    """k = 128 is past the cut's envelope (the fp64 pass's base row): refused, not run by the integer pass."""
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    S = _synth(128)
    ctx = twosd.SDContext(S.sp2, positions=S.positions)
    V = twosd.sdDualVertexSet(ctx)
    V.push_batch(np.random.default_rng(0).normal(size=(3, S.m2)))
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, SC.values(S, 5))
    with pytest.raises(TwoSDError) as ei:
        ctx.cut_debug_scores(epi.index, SC.X[0], 5, 3)
    assert ei.value.code == -5 and "k = 128" in str(ei.value)


# ---- pass equivalence ---------------------------------------------------------------------------------
def _built_at_x(name, nsrc):
    from sqlp_amd import smps, twosd
    inst = I.load(name)
    ctx = twosd.SDContext(inst["sp2"], inst["sto"])
    x = I.x_ev(name)
    ctx.compute_basis(x, smps.mean_values(inst["sto"]))
    src = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(src, I.sample(name, nsrc, 41))
    _, st, _ = twosd.solve_push(src, x, 0, nsrc)
    assert (st == 0).all()
    return inst, ctx, x, twosd.sdDualVertexSet(ctx)


def _three_passes(ctx, epi, x, tie_rel):
    from sqlp_amd import twosd
    got = {}
    for kind, env in PASS_ENV.items():
        with _env(**env):
            cut, mv, ma = twosd._build_cut(epi, x, tie_rel, want_argmax=True)
            got[kind] = (cut, mv, ma, ctx.cut_pass(), ctx.cut_pass_kind()[0], ctx.cut_stats())
        assert got[kind][4] == kind, (kind, got[kind][4])
        assert got[kind][3][0] == (1 if kind else 0)
    assert got[2][3][1] > got[0][3][1] > 0.0                 # the integer band is positive and wider than the fp64 one
    return got


def _check_against_oracle(got, a, b, omv, oma):
    for kind, (cut, mv, ma, _, _, _) in got.items():
        assert (ma == oma).all(), (kind, int((ma != oma).sum()))
        np.testing.assert_allclose(mv, omv, rtol=1e-12, atol=1e-9)
        assert cut.alpha == pytest.approx(a, rel=1e-8, abs=1e-8)
        np.testing.assert_allclose(cut.beta, b, rtol=1e-8, atol=1e-8 * (1 + np.abs(b).max()))


@pytest.mark.parametrize("name,N", [("storm", 6000), ("ssn", 5000)])
def test_three_passes_give_the_oracles_picks(name, N):
    """storm at x_EV with V built there (twin-rich, more than N/4 near ties) and ssn: the integer,
    fp32 and fp64 passes give the C oracle's pick for every scenario under both tie rules."""
    from oracle import cpu
    from sqlp_amd import twosd
    inst, ctx, x, V = _built_at_x(name, 8192)
    vals = I.sample(name, N, 43)
    w = np.random.default_rng(9).uniform(0.5, 1.5, size=N)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals, w)
    sp, Vm = inst["osp2"], V.matrix()
    if name == "storm":
        scores = (Vm @ (sp.r - sp.T @ x))[None, :] + (vals - sp.r[ctx.rows]) @ Vm[:, ctx.rows].T
        assert SC.near_ties(scores) > N // 4
    for tie_rel in (0.0, 1e-12):
        a, b, omv, oma = cpu.build_cut(sp.r, sp.T, x, Vm, ctx.rows, vals - sp.r[ctx.rows], w, tie_rel=tie_rel, nthreads=8)
        got = _three_passes(ctx, epi, x, tie_rel)
        _check_against_oracle(got, a, b, omv, oma)
        print(f"I8 {name} tie_rel {tie_rel}: bands int {got[2][3][1]:.4g} fp32 {got[1][3][1]:.4g} fp64 {got[0][3][1]:.4g}; "
              f"re-decided int {got[2][5][0]} fp32 {got[1][5][0]} fp64 {got[0][5][0]}")


def test_three_passes_importance_weighted_transship():
    from oracle import cpu
    from sqlp_amd import smps, twosd
    inst = I.load("transship")
    ctx = twosd.SDContext(inst["sp2"], inst["sto"])
    x = I.x_ev("transship")
    ctx.compute_basis(x, smps.mean_values(inst["sto"]))
    V = twosd.sdDualVertexSet(ctx)
    _, _, pis, st = ctx.solve_values(x, I.sample("transship", 2048, 3), want_pi=True)
    V.push_batch(pis[st == 0])
    sto = inst["sto"]
    mu = np.array([d[1] for d in sto.indep.values()])
    sd = np.sqrt([d[2] for d in sto.indep.values()])
    rng = np.random.default_rng(8)
    vals = rng.normal(mu, 1.5 * sd, size=(600, len(mu)))
    logw = (-0.5 * ((vals - mu) / sd) ** 2).sum(1) - (-0.5 * ((vals - mu) / (1.5 * sd)) ** 2).sum(1) + len(mu) * np.log(1.5)
    w = np.exp(logw)
    epi = twosd.sdEpigraph(ctx, 0.25, 0.0)
    twosd.add_scenarios(epi, vals, w)
    sp, Vm = inst["osp2"], V.matrix()
    for tie_rel in (0.0, 1e-12):
        a, b, omv, oma = cpu.build_cut(sp.r, sp.T, x, Vm, ctx.rows, vals - sp.r[ctx.rows], w, tie_rel=tie_rel)
        _check_against_oracle(_three_passes(ctx, epi, x, tie_rel), a, b, omv, oma)


@pytest.mark.parametrize("name,nsrc", [("ssn", 4096), ("storm", 8192)])
def test_three_passes_at_the_small_shapes(name, nsrc):
    """The steps the three passes share (unit arithmetic, tile end, block end) at the smallest shapes
    where they can go wrong: N in {1, 127, 129, 300} scenarios (the bounds of both scenario rows on
    either side of a tile) x |V| in {260, 33, 31, 1}.  |V| = 260 is 9 chunks: every tile runs as tail
    units of S = 2 vertex ranges into the tail logs and the merge, with the global histogram; |V| <= 33
    runs whole-tile units with the LDS histogram.  ssn is KB = 22: the fp64 pass at 3 blocks per CU
    without the held log entry, two integer k-steps; storm's fp64 pass runs at 2 blocks per CU with
    the held entry.  Every pass gives the C oracle's picks and cut under both tie rules."""
    from oracle import cpu
    from sqlp_amd import twosd
    inst, ctx, x, V = _built_at_x(name, nsrc)
    assert len(V) >= 260, len(V)
    sp = inst["osp2"]
    rng = np.random.default_rng(11)
    epis = {}
    for N in (1, 127, 129, 300):
        vals, w = I.sample(name, N, 50 + N), rng.uniform(0.5, 1.5, size=N)
        epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
        twosd.add_scenarios(epi, vals, w)
        epis[N] = (epi, vals, w)
    for nv in (260, 33, 31, 1):
        V.truncate(nv)
        Vm = V.matrix()
        for N, (epi, vals, w) in epis.items():
            for tie_rel in (0.0, 1e-12):
                a, b, omv, oma = cpu.build_cut(sp.r, sp.T, x, Vm, ctx.rows, vals - sp.r[ctx.rows], w, tie_rel=tie_rel)
                got = _three_passes(ctx, epi, x, tie_rel)
                _check_against_oracle(got, a, b, omv, oma)
        print(f"I8 small shapes {name} |V| {nv}: passes run {[got[k][4] for k in (2, 1, 0)]}, twins dropped {got[2][5][3]}")


# ---- full units and tail ranges -----------------------------------------------------------------------
@pytest.mark.parametrize("nv", [100, 260])
def test_full_units_and_tail_ranges_equal_the_fp32_pass(nv):
    """N = 131,201 is more than 3 blocks x 256 CUs x 128 scenarios: whole-tile units and a partial
    last round.  With |V| = 260 (9 chunks) the last round is cut into vertex ranges; with 100 it is
    not.  The integer pass against the fp32 pass on the GPU."""
    from sqlp_amd import twosd
    inst, ctx, x, V = _built_at_x("ssn", 4096)
    assert len(V) >= nv
    V.truncate(nv)
    N = 131201
    vals = I.sample("ssn", N, 47)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals)
    got = {}
    for kind in (2, 1):
        with _env(**PASS_ENV[kind]):
            got[kind] = twosd._build_cut(epi, x, 1e-12, want_argmax=True)
            assert ctx.cut_pass_kind()[0] == kind
    (c2, mv2, ma2), (c1, mv1, ma1) = got[2], got[1]
    assert np.array_equal(ma2, ma1)
    np.testing.assert_allclose(mv2, mv1, rtol=1e-12, atol=1e-9)
    assert c2.alpha == pytest.approx(c1.alpha, rel=1e-8, abs=1e-8)
    np.testing.assert_allclose(c2.beta, c1.beta, rtol=1e-8, atol=1e-8 * (1 + np.abs(c1.beta).max()))


# ---- fallbacks ----------------------------------------------------------------------------------------
def _ssn_small(nsrc=300):
    from sqlp_amd import smps, twosd
    inst = I.load("ssn")
    ctx = twosd.SDContext(inst["sp2"], inst["sto"])
    x = I.x_ev("ssn")
    ctx.compute_basis(x, smps.mean_values(inst["sto"]))
    V = twosd.sdDualVertexSet(ctx)
    _, _, pis, st = ctx.solve_values(x, I.sample("ssn", nsrc, 3), want_pi=True)
    V.push_batch(pis[st == 0])
    return inst, ctx, x, V


def test_fallbacks():
    from sqlp_amd import twosd
    inst, ctx, x, V = _ssn_small()
    vals = I.sample("ssn", 2000, 73)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals)
    twosd._build_cut(epi, x, 0.0, want_argmax=True)
    assert ctx.cut_pass_kind()[0] == 2                      # the default
    with _env(TWOSD_CUT_I8="0"):
        twosd._build_cut(epi, x, 0.0, want_argmax=True)
        assert ctx.cut_pass_kind()[0] == 1 and ctx.cut_pass()[0] == 1
    # a NaN delta: the parent's pass (fp32) and its outputs, bit for bit
    bad = vals.copy()
    bad[17, 5] = np.nan
    epi_n = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi_n, bad)
    cut_d, mv_d, ma_d = twosd._build_cut(epi_n, x, 0.0, want_argmax=True)
    assert ctx.cut_pass_kind()[0] != 2
    with _env(TWOSD_CUT_I8="0"):
        cut_p, mv_p, ma_p = twosd._build_cut(epi_n, x, 0.0, want_argmax=True)
    assert np.array_equal(ma_d, ma_p) and np.array_equal(mv_d.view(np.uint64), mv_p.view(np.uint64))
    assert np.array_equal(np.float64(cut_d.alpha).view(np.uint64), np.float64(cut_p.alpha).view(np.uint64))
    assert np.array_equal(cut_d.beta.view(np.uint64), cut_p.beta.view(np.uint64))
    # the 1e32-scaled vertex of the envelope test: the fp64 pass
    big = V.matrix()[1].copy()
    big[ctx.rows] *= 1e32
    V.push_batch(big[None, :])
    twosd._build_cut(epi, x, 0.0, want_argmax=True)
    assert ctx.cut_pass_kind()[0] == 0 and ctx.cut_pass()[0] == 0


# ---- split cut ----------------------------------------------------------------------------------------
def test_split_cut_equals_the_unsplit_cut_bit_for_bit():
    """twosd_cut_partial over two halves + finalize == the unsplit partial + finalize on the integer pass."""
    import torch
    from sqlp_amd import twosd
    inst, ctx, x, V = _ssn_small(1024)
    vals = I.sample("ssn", 2000, seed=21)
    w = np.random.default_rng(1).uniform(0.5, 1.5, size=2000)
    full = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(full, vals, w)
    halves = [twosd.sdEpigraph(ctx, 1.0, 0.0) for _ in range(2)]
    twosd.add_scenarios(halves[0], vals[:900], w[:900])
    twosd.add_scenarios(halves[1], vals[900:], w[900:])
    nu, nf = ctx.cut_partial_len()
    dev = torch.device("cuda", 0)
    H = [torch.zeros(nu, dtype=torch.int64, device=dev) for _ in range(2)]
    Sm = [torch.zeros(nf, dtype=torch.float64, device=dev) for _ in range(2)]
    hist1 = torch.zeros(nu, dtype=torch.int64, device=dev)
    sums1 = torch.zeros(nf, dtype=torch.float64, device=dev)
    ctx.cut_partial(full, x, 1e-12, w.sum(), hist1.data_ptr(), sums1.data_ptr())
    assert ctx.cut_pass_kind()[0] == 2
    for e in range(2):
        ctx.cut_partial(halves[e], x, 1e-12, w.sum(), H[e].data_ptr(), Sm[e].data_ptr())
        assert ctx.cut_pass_kind()[0] == 2
    torch.cuda.synchronize()
    hist, sums = H[0] + H[1], Sm[0] + Sm[1]
    assert torch.equal(hist, hist1)
    a1, b1 = ctx.cut_finalize(x, hist1.data_ptr(), sums1.data_ptr())
    a, b = ctx.cut_finalize(x, hist.data_ptr(), sums.data_ptr())
    print(f"I8 split: alpha {a!r} vs {a1!r}, max |beta diff| {np.abs(b - b1).max():.3e}")
    assert a == a1 and np.array_equal(b, b1)
