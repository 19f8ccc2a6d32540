"""Tail handles (sqlp_amd/csrc/risk.hip: twosd_tail_keep / _info / _get) and their re-formation
under bootstrap weights (boot_kernel.hip: the LIST instantiations of boot_weight_kernel,
boot_hist_kernel and boot_reform_kernel) against tests/boot_ref.py: the reference of a tail handle's row b is
boot_ref.reform(..., c = counts[:, b] * (max_val > eta)), the tail set taken on the host from the
max_val the cut call returned.

Tolerance: the project's cut tolerance, tests/test_gpu_bootstrap._close (1e-8 (1 + |ref|), beta
against its largest entry); integer-derived outputs (weight_mark, total_weight) as that file
compares them.  Instances: lands, transship (two epigraphs, non-unit weights), randT, boxed
(c0 != 0) and the synthetic a (k = 1), k87, k88, k119, k120 (two elements per lane), 300 scenarios
kept in three stages of 100 / 200 / 300 with the vertex set growing in between.

lands' scenarios take three values, so its cut has three distinct scores: its VaR at 0.8 and 0.95
is the largest score and the strict tail above it is empty.  "The three quantile tails are
non-empty and differ" is asserted on every instance whose scores are continuous (all but lands,
which is asserted to have at most three scores and nested tails)."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import boot_ref as BR
from tests import instances as I
from tests import synth_cases as SC
from tests.test_gpu_bootstrap import SEED, STAGES, _close, _context, _template_arrays
from tests.test_gpu_risk_tail import _env

pytestmark = pytest.mark.gpu

NAMES = ["lands", "transship", "randT", "boxed", "a", "k87", "k88", "k119", "k120"]
DISCRETE = {"lands"}
LEVELS = (0.5, 0.8, 0.95)

_BUILT = {}


@pytest.fixture(scope="module", autouse=True)
def _close_shared_contexts():
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


def _keep(epi, eta, mv, ma):
    """A tail handle of the last cut at eta with what the host expects of it."""
    from sqlp_amd import twosd
    th = twosd.keep_tail_of_last_cut(epi, eta)
    return SimpleNamespace(h=th, eta=float(eta), flag=mv > eta, scen=np.flatnonzero(mv > eta), arg=ma)


def _build(name):
    """test_gpu_bootstrap._build with, per kept cut, its scores, the tail cut and a tail handle at
    the cut's 0.8 quantile; the last cut of each epigraph also keeps handles at the 0.5 and 0.95
    quantiles, below every score and above every score."""
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
            mv, ma = mv.copy(), ma.copy()
            h = twosd.keep_picks_of_last_cut(epi)
            eta = twosd.cut_quantile(epi, 0.8).var
            K = SimpleNamespace(cut=cut, mv=mv, arg=ma, h=h, n=hi, nv=len(V), tail=twosd.cut_tail(epi, eta),
                                t=_keep(epi, eta, mv, ma), at={})
            if j == len(STAGES) - 1:
                for lvl in LEVELS:
                    K.at[lvl] = _keep(epi, twosd.cut_quantile(epi, lvl).var, mv, ma)
                K.at["below"] = _keep(epi, float(mv.min()) - 1.0, mv, ma)
                K.at["above"] = _keep(epi, float(mv.max()), mv, ma)      # strict: exactly the largest score is outside
            kept.append(K)
        epis.append(SimpleNamespace(epi=epi, kept=kept, dv=vals - ctx.template_values, w=w))
    return SimpleNamespace(ctx=ctx, x=x, r=r, T=T, c0=c0, V=V, epis=epis)


def _ref(B, E, handles, M, cnt):
    """boot_ref's rows of `handles` -- (picks, n, flag or None) each -- under the counts cnt (N x M)."""
    ctx = B.ctx
    Vm = B.V.matrix()
    N = len(E.w)
    H = len(handles)
    a = np.zeros((M + 1, H)); b = np.zeros((M + 1, H, ctx.n1)); wm = np.zeros((M + 1, H)); tw = np.zeros(M + 1)
    for row in range(M + 1):
        c = np.ones(N) if row == 0 else cnt[:, row - 1].astype(np.float64)
        tw[row] = float(np.sum(c * E.w))
        for j, (arg, n, flag) in enumerate(handles):
            cj = c[:n] if flag is None else c[:n] * flag[:n]
            a[row, j], b[row, j], wm[row, j] = BR.reform(B.r, B.T, B.c0, ctx.rows, ctx.cols, Vm, E.dv, E.w, arg[:n], cj)
    return a, b, wm, tw


def _check(R, ref, what):
    a, b, wm, tw = ref
    _close(R.alpha, a, f"{what} alpha")
    _close(R.beta, b, f"{what} beta")
    _close(R.weight_mark, wm, f"{what} weight_mark")
    _close(R.total_weight, tw, f"{what} total_weight")


def _same_bits(Ra, Rb):
    for f in ("alpha", "beta", "weight_mark", "total_weight"):
        np.testing.assert_array_equal(getattr(Ra, f), getattr(Rb, f))


# ---------------------------------------------------------------- the handle itself
@pytest.mark.parametrize("name", NAMES)
def test_handle_contents(name):
    from sqlp_amd import twosd
    B = _built(name)
    for E in B.epis:
        K = E.kept[-1]
        nts = {}
        for Kc, key, t in [(K, key, t) for key, t in K.at.items()] + [(Kj, "stage", Kj.t) for Kj in E.kept]:
            scen, pick = twosd.tail_get(B.ctx, t.h)
            np.testing.assert_array_equal(scen, np.flatnonzero(Kc.mv > t.eta))
            np.testing.assert_array_equal(pick, Kc.arg[scen])
            info = twosd.tail_info(B.ctx, t.h)
            assert info == twosd.TailInfo(E.epi.index, Kc.n, Kc.nv, len(scen), t.eta), (name, key, info)
            assert twosd.picks_info(B.ctx, t.h) == (E.epi.index, Kc.n, Kc.nv)
            nts[key] = len(scen)
        n50, n80, n95, nall, nnone = (nts[key] for key in (0.5, 0.8, 0.95, "below", "above"))
        assert nall == K.n and nnone == 0
        assert n50 >= n80 >= n95
        if name in DISCRETE:
            assert len(np.unique(K.mv)) <= 3
        else:
            assert n50 > n80 > n95 > 0, (name, nts)


@pytest.mark.parametrize("name", NAMES)
def test_identity_row_is_the_tail_cut(name):
    from sqlp_amd import twosd
    B = _built(name)
    for E in B.epis:
        R = twosd.reform_cuts(E.epi, [K.t.h for K in E.kept], 0, SEED)
        assert R.alpha.shape == (1, 3)
        for j, K in enumerate(E.kept):
            _close(R.alpha[0, j], K.tail.alpha, f"{name} alpha[{j}]")
            _close(R.beta[0, j], K.tail.beta, f"{name} beta[{j}]")
            _close(R.weight_mark[0, j], K.tail.tail_weight, f"{name} tail_weight[{j}]")
        _close(R.total_weight[0], E.epi.total_scenario_weight, f"{name} total weight")


@pytest.mark.parametrize("name", NAMES)
def test_full_tail_is_the_pick_handle(name):
    from sqlp_amd import twosd
    B = _built(name)
    for e, E in enumerate(B.epis):
        K = E.kept[-1]
        R = twosd.reform_cuts(E.epi, [K.h, K.at["below"].h], 33, SEED + e, index_offset=7)
        np.testing.assert_array_equal(R.weight_mark[:, 1], R.weight_mark[:, 0])
        _close(R.alpha[:, 1], R.alpha[:, 0], f"{name} full tail alpha")
        _close(R.beta[:, 1], R.beta[:, 0], f"{name} full tail beta")


@pytest.mark.parametrize("name", NAMES)
def test_empty_tail_is_the_zero_cut(name):
    from sqlp_amd import twosd
    B = _built(name)
    for E in B.epis:
        K = E.kept[-1]
        assert twosd.tail_info(B.ctx, K.at["above"].h).nt == 0
        alone = twosd.reform_cuts(E.epi, [K.at["above"].h], 33, SEED)
        mixed = twosd.reform_cuts(E.epi, [K.t.h, K.at["above"].h, K.h], 33, SEED)
        for R, j in ((alone, 0), (mixed, 1)):
            assert not R.alpha[:, j].any() and not R.beta[:, j].any() and not R.weight_mark[:, j].any()
        assert (alone.total_weight > 0.0).all()
        np.testing.assert_array_equal(alone.total_weight, mixed.total_weight)


# ---------------------------------------------------------------- replicates
@pytest.mark.parametrize("M,off", [(1, 0), (33, 1000), (64, 0)])
@pytest.mark.parametrize("name", NAMES)
def test_replicates_match_restatement(name, M, off):
    from sqlp_amd import twosd
    B = _built(name)
    for e, E in enumerate(B.epis):
        K0, K1, K2 = E.kept
        R = twosd.reform_cuts(E.epi, [K0.t.h, K1.h, K1.t.h, K2.t.h, K2.at[0.5].h], M, SEED + e, index_offset=off)
        cnt = BR.counts(SEED + e, off, len(E.w), M)
        ref = _ref(B, E, [(K0.arg, K0.n, K0.t.flag), (K1.arg, K1.n, None), (K1.arg, K1.n, K1.t.flag), (K2.arg, K2.n, K2.t.flag),
                          (K2.arg, K2.n, K2.at[0.5].flag)], M, cnt)
        _check(R, ref, f"{name} M={M}")


def _single(name, N, G=1):
    """A fresh context with one epigraph of the first N scenarios and its cut: (B, E, epi, mv, ma, h)."""
    from sqlp_amd import twosd
    ctx, x, data = _context(name)
    vals, w = data[0][0][:N], np.random.default_rng(9).uniform(0.5, 1.5, size=N)
    r, T, c0 = _template_arrays(ctx)
    V = twosd.sdDualVertexSet(ctx)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals, w)
    twosd.solve_push(epi, x, 0, N)
    cut, mv, ma = twosd._build_cut(epi, x, 0.0, want_argmax=True)
    h = twosd.keep_picks_of_last_cut(epi)
    B = SimpleNamespace(ctx=ctx, r=r, T=T, c0=c0, V=V, x=x)
    E = SimpleNamespace(w=w, dv=vals - ctx.template_values, vals=vals)
    return B, E, epi, mv.copy(), ma.copy(), h


@pytest.mark.parametrize("nt", [1, 63, 64, 65])
@pytest.mark.parametrize("name", ["boxed", "k88"])
def test_lists_around_one_tile(name, nt):
    """N = 130 scenarios with distinct scores and eta at the score that leaves exactly nt above it:
    a list of one entry, a partial tile, exactly one, one and an entry.  The list is the same under
    any grid of the compaction kernels."""
    from sqlp_amd import twosd
    N = 130
    B, E, epi, mv, ma, h = _single(name, N)
    srt = np.sort(mv)
    assert len(np.unique(srt)) == N
    eta = float(srt[N - nt - 1])
    flag = mv > eta
    assert int(flag.sum()) == nt                           # before the device call
    th = twosd.keep_tail_of_last_cut(epi, eta)
    scen, pick = twosd.tail_get(B.ctx, th)
    np.testing.assert_array_equal(scen, np.flatnonzero(flag))
    np.testing.assert_array_equal(pick, ma[flag])
    for blocks in ("1", "3"):
        with _env(TWOSD_RISK_BLOCKS=blocks):
            t2 = twosd.keep_tail_of_last_cut(epi, eta)
        s2, p2 = twosd.tail_get(B.ctx, t2)
        np.testing.assert_array_equal(s2, scen)
        np.testing.assert_array_equal(p2, pick)
    for M, off in [(1, 1000), (33, 0), (64, 1000)]:
        R = twosd.reform_cuts(epi, [th, h], M, SEED, index_offset=off)
        ref = _ref(B, E, [(ma, N, flag), (ma, N, None)], M, BR.counts(SEED, off, N, M))
        _check(R, ref, f"{name} nt={nt} M={M}")
    B.ctx.close()


def test_list_past_eight_shards():
    """lands at N = 2500 with eta below every score: a list of 2500 entries, 40 tiles in 10 shards,
    more than the eight segments the shards' partials are summed in."""
    from sqlp_amd import twosd
    N, M = 2500, 1
    ctx, x, _ = _context("lands")
    vals, w = I.sample("lands", N, 3), np.random.default_rng(9).uniform(0.5, 1.5, size=N)
    r, T, c0 = _template_arrays(ctx)
    V = twosd.sdDualVertexSet(ctx)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals, w)
    twosd.solve_push(epi, x, 0, N)
    cut, mv, ma = twosd._build_cut(epi, x, 0.0, want_argmax=True)
    eta = float(np.sort(mv)[0]) - 1.0
    flag = mv > eta
    assert int(flag.sum()) >= 2304                         # 36 tiles: nine shards or more
    th = twosd.keep_tail_of_last_cut(epi, eta)
    assert twosd.tail_info(ctx, th).nt == int(flag.sum())
    B = SimpleNamespace(ctx=ctx, r=r, T=T, c0=c0, V=V)
    E = SimpleNamespace(w=w, dv=vals - ctx.template_values)
    R = twosd.reform_cuts(epi, [th], M, SEED)
    _check(R, _ref(B, E, [(ma, N, flag)], M, BR.counts(SEED, 0, N, M)), f"lands N={N}")
    _close(R.alpha[0, 0], cut.alpha, "identity alpha")
    ctx.close()


# ---------------------------------------------------------------- grouped counts
@pytest.mark.parametrize("G", [2, 64])
@pytest.mark.parametrize("name", ["boxed", "k119"])
def test_grouped_counts(name, G):
    """Under a plan the count of a list entry is its scenario's group's: antithetic pairs and LHS
    groups of 64 (a 64-entry tile of the list spans several groups either way), one and two
    elements per lane."""
    from sqlp_amd import twosd
    plan = twosd.Sampling.antithetic() if G == 2 else twosd.Sampling.lhs(64)
    N, M, off = 256, 33, 10 * G
    B, E, epi, mv, ma, h = _single(name, N)
    eta = float(np.sort(mv)[N // 2])
    flag = mv > eta
    assert 64 < int(flag.sum()) < N
    th = twosd.keep_tail_of_last_cut(epi, eta)
    R = twosd.reform_cuts(epi, [th, h], M, SEED, index_offset=off, sampling=plan)
    cnt = np.repeat(BR.counts(SEED, off // G, N // G, M), G, axis=0)
    _check(R, _ref(B, E, [(ma, N, flag), (ma, N, None)], M, cnt), f"{name} G={G}")
    _same_bits(R, twosd.reform_cuts(epi, [th, h], M, SEED, index_offset=off, sampling=plan))
    B.ctx.close()


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("name", ["transship", "k119"])
def test_same_bits_every_call_and_per_handle(name):
    from sqlp_amd import twosd
    B = _built(name)
    E = B.epis[-1]
    hs = [E.kept[0].t.h, E.kept[1].h, E.kept[2].t.h, E.kept[2].at["above"].h, E.kept[2].at[0.5].h]
    R1 = twosd.reform_cuts(E.epi, hs, 33, SEED, index_offset=5)
    _same_bits(R1, twosd.reform_cuts(E.epi, hs, 33, SEED, index_offset=5))
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
    _, mv, ma = twosd._build_cut(epi, x, 0.0, want_argmax=True)
    eta = float(np.sort(mv)[(7 * N) // 10])
    assert 0 < (mv[:half] > eta).sum() and 0 < (mv[half:] > eta).sum()
    h = twosd.keep_picks_of_last_cut(epi)
    th = twosd.keep_tail_of_last_cut(epi, eta)
    total = epi.total_scenario_weight
    whole = twosd.reform_cuts(epi, [th, h], M, SEED)
    nu, nf = twosd.reform_partial_len(ctx, [th, h], M)

    def bufs():
        return torch.zeros(nu, dtype=torch.int64, device="cuda"), torch.zeros(nf, dtype=torch.float64, device="cuda")
    u0, f0 = bufs()
    twosd.reform_partial(epi, [th, h], M, SEED, 0, total, u0.data_ptr(), f0.data_ptr())
    ranks = []
    for rk in range(2):
        c2, _, _ = _context("transship")
        V2 = twosd.sdDualVertexSet(c2)
        V2.push_batch(V.matrix())
        assert V2.fingerprint() == V.fingerprint()
        e2 = twosd.sdEpigraph(c2, 1.0, 0.0)
        sl = slice(rk * half, (rk + 1) * half)
        twosd.add_scenarios(e2, vals[sl], w[sl])
        _, mv2, ma2 = twosd._build_cut(e2, x, 0.0, want_argmax=True)
        np.testing.assert_array_equal(ma2, ma[sl])
        np.testing.assert_array_equal(mv2 > eta, mv[sl] > eta)
        h2 = twosd.keep_picks_of_last_cut(e2)
        t2 = twosd.keep_tail_of_last_cut(e2, eta)
        assert twosd.reform_partial_len(c2, [t2, h2], M) == (nu, nf)
        u, f = bufs()
        twosd.reform_partial(e2, [t2, h2], M, SEED, rk * half, total, u.data_ptr(), f.data_ptr())
        ranks.append((c2, [t2, h2], u, f))
    u = ranks[0][2] + ranks[1][2]      # rank order
    f = ranks[0][3] + ranks[1][3]
    torch.cuda.synchronize()
    assert torch.equal(u, u0)          # the totals, the W words and the per-vertex weights: integers, exact under the split
    for c2, hs2, _, _ in ranks:
        R = twosd.reform_finalize(c2, hs2, M, total, u.data_ptr(), f.data_ptr())
        np.testing.assert_array_equal(R.weight_mark, whole.weight_mark)
        np.testing.assert_array_equal(R.total_weight, whole.total_weight)
        _close(R.alpha, whole.alpha, "split alpha")
        _close(R.beta, whole.beta, "split beta")
    for c2, _, _, _ in ranks:
        c2.close()
    ctx.close()


# ---------------------------------------------------------------- refusals and lifetime
def test_refusals_and_lifetime():
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    inst = I.load("lands")
    ctx, x, data = _context("lands")
    vals = data[0][0]
    V = twosd.sdDualVertexSet(ctx)
    ea, eb = twosd.sdEpigraph(ctx, 0.5, 0.0), twosd.sdEpigraph(ctx, 0.5, 0.0)
    twosd.add_scenarios(ea, vals[:40])
    twosd.add_scenarios(eb, vals[40:80])

    def refused(code, text, f, *args, **kw):
        with pytest.raises(TwoSDError) as ei:
            f(*args, **kw)
        assert ei.value.code == code and text in str(ei.value), str(ei.value)
    twosd.solve_push(ea, x, 0, 40)
    nv0 = len(V)
    ca = twosd.build_sasa_cut(ea, x, V, keep_picks=True)
    refused(-1, "eta is NaN", twosd.keep_tail_of_last_cut, ea, float("nan"))
    ta = twosd.cut_tail(ea, -1.0, keep=True)
    assert ta.picks in ea._pick_handles and twosd.tail_info(ctx, ta.picks).nt == 40
    twosd.solve_push(eb, 1.2 * x, 0, 40)
    twosd.build_sasa_cut(eb, 1.2 * x, V)
    tb = twosd.keep_tail_of_last_cut(eb, -1.0)
    assert twosd.picks_count(ctx) == 3 and twosd.picks_info(ctx, tb)[2] == len(V) > nv0
    refused(-3, f"the last cut was built on epigraph {eb.index}, not {ea.index}", twosd.keep_tail_of_last_cut, ea, 0.0)
    refused(-1, f"belongs to epigraph {eb.index}, not {ea.index}", twosd.reform_cuts, ea, [ta, tb], 4, SEED)
    refused(-1, "twosd_tail_get", twosd.picks_get, ctx, ta.picks)
    refused(-1, "not a tail handle", twosd.tail_info, ctx, ca.picks)
    refused(-1, "not a tail handle", twosd.tail_get, ctx, ca.picks)
    # release_unused_picks treats it as a pick handle of the epigraph
    assert twosd.release_unused_picks(eb, keep=[tb]) == 0 and twosd.release_unused_picks(eb) == 1
    refused(-1, "does not exist", twosd.tail_info, ctx, tb)
    tb = twosd.keep_tail_of_last_cut(eb, -1.0)
    # truncation below a handle's nv: tb (built over more vertices) dies, ta lives when nv0 stays
    V.truncate(nv0)
    refused(-3, "truncated", twosd.reform_cuts, eb, [tb], 4, SEED)
    refused(-3, "truncated", twosd.tail_get, ctx, tb)
    assert twosd.reform_cuts(ea, [ta, ca], 4, SEED).alpha.shape == (5, 2)
    refused(-3, "no cut to read the picks of", twosd.keep_tail_of_last_cut, eb, 0.0)   # the vertex set was reset since
    twosd.picks_release(ctx, tb)
    refused(-1, "does not exist", twosd.picks_release, ctx, tb)
    refused(-1, "does not exist", twosd.reform_cuts, eb, [tb], 4, SEED)
    # a new template drops every handle
    assert twosd.picks_count(ctx) == 2
    ctx._set_problem(inst["sp2"], inst["sto"])
    assert twosd.picks_count(ctx) == 0
    refused(-1, "does not exist", twosd.tail_info, ctx, ta.picks)
    refused(-1, "does not exist", twosd.reform_cuts, ea, [ta], 4, SEED)
    ctx.close()


def test_k_128_is_refused():
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    S = SC.synth_template(160, 400, 128, seed=171, amp=0.2)
    ctx = twosd.SDContext(S.sp2, positions=S.positions)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    with pytest.raises(TwoSDError) as e:
        twosd.keep_tail_of_last_cut(epi, 0.0)
    assert e.value.code == -5 and "127" in str(e.value)
    ctx.close()
