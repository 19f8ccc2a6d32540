"""The bootstrap of whole groups on an epigraph filled from a variance-reduced stream (DESIGN.md
§5.8 / §5.9): the grouped instantiations of sqlp_amd/csrc/boot_kernel.hip behind the _vr entry
points against the numpy restatement tests/boot_ref.py fed with the repeated counts of the global
group indices, the sharded wrapper, the refusals, and the stopping rule end to end.

Tolerance: tests/test_gpu_bootstrap.py's (_close: 1e-8 (1 + |reference|) for alpha, beta and the
weights); counts, weight_mark and total_weight bit for bit where that module compares bits.
Shapes: stages at N_j = L, 2 L, 3 L scenarios with L per plan -- G = 2: 100; G = 3: 99 (297
scenarios: groups straddle the 64-scenario tile and the 4-wave boundaries); G = 64: 64; G = 100:
100; G = 256: 256 (768 scenarios: a group spans four tiles, the wave-uniform kernel) -- on lands,
transship (weighted, two epigraphs) and the synthetic k88 / k120 (one and two elements per lane)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests import boot_ref as BR
from tests import instances as I
from tests import synth_cases as SC
from tests import vr_ref as R
from tests.test_gpu_bootstrap import SEED, _close, _template_arrays

pytestmark = pytest.mark.gpu

NAMES = ["lands", "transship", "k88", "k120"]
PLANS = {"anti": (2, 100), "lhs3": (3, 99), "lhs64": (64, 64), "lhs100": (100, 100), "lhs256": (256, 256)}   # (G, L)


def _plan(G):
    from sqlp_amd import twosd
    return twosd.Sampling.antithetic() if G == 2 else twosd.Sampling.lhs(G)


def _gcounts(seed, first, count, M, G):
    """The grouped counts of scenarios [first, first + count): the i.i.d. counts of the global group
    indices, every member carrying its group's."""
    assert first % G == 0 and count % G == 0
    return np.repeat(BR.counts(seed, first // G, count // G, M), G, axis=0)


def _context(name, N):
    """(ctx, x, [(values, weights) per epigraph]) with N scenarios per epigraph (test_gpu_bootstrap's
    _context at another size)."""
    from sqlp_amd import smps, twosd
    rng = np.random.default_rng(7)
    if name in ("lands", "transship"):
        inst = I.load(name)
        ctx = twosd.SDContext(inst["sp2"], inst["sto"])
        x = I.x_ev(name)
        ctx.compute_basis(x, smps.mean_values(inst["sto"]))
        if name == "lands":
            return ctx, x, [(I.sample(name, N, 3), np.ones(N))]
        return ctx, x, [(I.sample(name, N, 3 + e), rng.uniform(0.5, 1.5, size=N)) for e in range(2)]
    S = SC.template(name)
    ctx = twosd.SDContext(S.sp2, positions=S.positions)
    ctx.compute_basis(SC.X[0], SC.values(S)[0])
    return ctx, SC.X[0], [(SC.values(S, N), SC.weights(N))]


def _build(name, stages):
    """As test_gpu_bootstrap's _build: per epigraph one cut kept after each stage [lo, hi), new vertices
    pushed before each."""
    from sqlp_amd import twosd
    ctx, x, data = _context(name, stages[-1][1])
    r, T, c0 = _template_arrays(ctx)
    V = twosd.sdDualVertexSet(ctx)
    epis = []
    for vals, w in data:
        epi = twosd.sdEpigraph(ctx, 1.0 / len(data), 0.0)
        kept = []
        for j, (lo, hi) in enumerate(stages):
            twosd.add_scenarios(epi, vals[lo:hi], w[lo:hi])
            xs = x * (1.0 + 0.03 * j)
            twosd.solve_push(epi, xs, lo, hi - lo)
            cut, mv, ma = twosd._build_cut(epi, xs, 0.0, want_argmax=True)
            kept.append(SimpleNamespace(cut=cut, arg=ma.copy(), h=twosd.keep_picks_of_last_cut(epi), n=hi, nv=len(V)))
        epis.append(SimpleNamespace(epi=epi, kept=kept, dv=vals - ctx.template_values, w=w))
    return SimpleNamespace(ctx=ctx, x=x, r=r, T=T, c0=c0, V=V, epis=epis)


_BUILT = {}


def _built(name, which):
    if (name, which) not in _BUILT:
        L = PLANS[which][1]
        _BUILT[name, which] = _build(name, [(0, L), (L, 2 * L), (2 * L, 3 * L)])
    return _BUILT[name, which]


@pytest.fixture(scope="module", autouse=True)
def _close_shared_contexts():
    yield
    for B in _BUILT.values():
        B.ctx.close()
    _BUILT.clear()
    BR.counts.cache_clear()
    import gc
    gc.collect()


def _ref_rows(B, E, M, seed, off, G):
    """boot_ref's (alpha, beta, weight_mark, total_weight) in reform_cuts' layout under the grouped counts."""
    ctx, Vm, N, H = B.ctx, B.V.matrix(), len(E.w), len(E.kept)
    cnt = _gcounts(seed, off, N, M, G).astype(np.float64)
    a = np.zeros((M + 1, H)); b = np.zeros((M + 1, H, ctx.n1)); wm = np.zeros((M + 1, H)); tw = np.zeros(M + 1)
    for row in range(M + 1):
        c = None if row == 0 else cnt[:, row - 1]
        tw[row] = float(np.sum((np.ones(N) if c is None else c) * E.w))
        for j, K in enumerate(E.kept):
            a[row, j], b[row, j], wm[row, j] = BR.reform(B.r, B.T, B.c0, ctx.rows, ctx.cols, Vm, E.dv, E.w, K.arg,
                                                         None if c is None else c[:K.n])
    return a, b, wm, tw


def _check(R_, ref, what):
    for got, want, f in zip((R_.alpha, R_.beta, R_.weight_mark, R_.total_weight), ref, ("alpha", "beta", "weight_mark", "total_weight")):
        _close(got, want, f"{what} {f}")


def _same_bits(Ra, Rb):
    for f in ("alpha", "beta", "weight_mark", "total_weight"):
        np.testing.assert_array_equal(getattr(Ra, f), getattr(Rb, f))


# ---------------------------------------------------------------- 1. counts
@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("M", [1, 5, 64])
@pytest.mark.parametrize("G", [2, 3, 64, 256])
def test_counts_bit_equal(G, M, far):
    from sqlp_amd import twosd
    ctx = _built("lands", "anti").ctx
    first = -(-2 ** 33 // G) * G if far else 0          # far: for G = 2 the group index passes 32 bits
    count = 384 if G == 2 else 3 * G
    plan = _plan(G)
    got = twosd.bootstrap_counts(ctx, M, SEED, first, count, sampling=plan)
    np.testing.assert_array_equal(got, _gcounts(SEED, first, count, M, G))
    assert (got.reshape(count // G, G, M) == got[::G, None, :]).all()       # every member: its group's count
    cut = G * (count // G // 3)
    two = np.vstack([twosd.bootstrap_counts(ctx, M, SEED, first, cut, sampling=plan),
                     twosd.bootstrap_counts(ctx, M, SEED, first + cut, count - cut, sampling=plan)])
    np.testing.assert_array_equal(two, got)


# ---------------------------------------------------------------- 2. re-formed cuts against the restatement
@pytest.mark.parametrize("which", list(PLANS))
@pytest.mark.parametrize("name", NAMES)
def test_replicates_match_restatement(name, which):
    from sqlp_amd import twosd
    G = PLANS[which][0]
    B = _built(name, which)
    for M in (1, 33, 64):
        for off in (0, 5 * G * 64 + G):
            for e, E in enumerate(B.epis):
                got = twosd.reform_cuts(E.epi, [K.h for K in E.kept], M, SEED + e, index_offset=off, sampling=_plan(G))
                _check(got, _ref_rows(B, E, M, SEED + e, off, G), f"{name} {which} M={M} off={off}")


# ---------------------------------------------------------------- 3. around one tile
@pytest.mark.parametrize("G,N", [(2, 2), (2, 62), (2, 64), (2, 66), (2, 128), (2, 130), (3, 3), (3, 63), (3, 66)])
@pytest.mark.parametrize("name", ["transship", "k120"])
def test_replicates_around_one_tile(name, G, N):
    from sqlp_amd import twosd
    B = _build(name, [(0, N)])
    E = B.epis[0]
    for off in (0, 5 * G * 64 + G):
        got = twosd.reform_cuts(E.epi, [E.kept[0].h], 17, SEED, index_offset=off, sampling=_plan(G))
        _check(got, _ref_rows(B, E, 17, SEED, off, G), f"{name} G={G} N={N} off={off}")
    _close(got.alpha[0, 0], E.kept[0].cut.alpha, "identity alpha")
    B.ctx.close()


def test_replicates_past_eight_shards():
    """lands in antithetic pairs at N = 2500: 10 shards, more than the eight summing segments."""
    from sqlp_amd import twosd
    B = _build("lands", [(0, 2500)])
    E = B.epis[0]
    got = twosd.reform_cuts(E.epi, [E.kept[0].h], 1, SEED, sampling=_plan(2))
    _check(got, _ref_rows(B, E, 1, SEED, 0, 2), "lands G=2 N=2500 M=1")
    B.ctx.close()


# ---------------------------------------------------------------- 4. the group property
@pytest.mark.parametrize("which", ["anti", "lhs3", "lhs256"])
def test_total_weight_is_counts_times_group_weights(which):
    """transship's weights differ inside every group; total_weight[1 + b] = sum over the groups of count x
    (sum of the members' integer weights q_s = rn(w_s 2^58 / total)), in integers, scaled back as the
    library does: bit for bit."""
    from sqlp_amd import twosd
    G = PLANS[which][0]
    B = _built("transship", which)
    E = B.epis[1]
    N, M, off = len(E.w), 64, 5 * G * 64 + G
    assert (E.w.reshape(-1, G).std(axis=1) > 0).all()
    plan = _plan(G)
    got = twosd.reform_cuts(E.epi, [K.h for K in E.kept], M, SEED, index_offset=off, sampling=plan)
    cnt = twosd.bootstrap_counts(B.ctx, M, SEED, off, N, sampling=plan)
    total = E.epi.total_scenario_weight
    scale = 2.0 ** 58 / total
    q = [int(np.rint(w * scale)) for w in E.w]
    qg = [sum(q[i:i + G]) for i in range(0, N, G)]
    wunit = total / 2.0 ** 58
    want = [float(sum(q)) * wunit] + [float(sum(int(cnt[g * G, b]) * qg[g] for g in range(N // G))) * wunit for b in range(M)]
    np.testing.assert_array_equal(got.total_weight, np.array(want))
    for j, K in enumerate(E.kept):                     # W_jb of a handle: the same sum over its first N_j / G groups
        wj = [float(sum(int(cnt[g * G, b]) * qg[g] for g in range(K.n // G))) * wunit for b in range(M)]
        np.testing.assert_array_equal(got.weight_mark[1:, j], np.array(wj))


# ---------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("name,which", [("transship", "lhs3"), ("k120", "lhs256"), ("k88", "anti")])
def test_same_bits_every_call_and_per_handle(name, which):
    from sqlp_amd import twosd
    G = PLANS[which][0]
    E = _built(name, which).epis[-1]
    hs = [K.h for K in E.kept]
    R1 = twosd.reform_cuts(E.epi, hs, 33, SEED, index_offset=3 * G, sampling=_plan(G))
    _same_bits(R1, twosd.reform_cuts(E.epi, hs, 33, SEED, index_offset=3 * G, sampling=_plan(G)))
    for j, h in enumerate(hs):
        Rj = twosd.reform_cuts(E.epi, [h], 33, SEED, index_offset=3 * G, sampling=_plan(G))
        np.testing.assert_array_equal(Rj.alpha[:, 0], R1.alpha[:, j])
        np.testing.assert_array_equal(Rj.beta[:, 0], R1.beta[:, j])
        np.testing.assert_array_equal(Rj.weight_mark[:, 0], R1.weight_mark[:, j])
        np.testing.assert_array_equal(Rj.total_weight, R1.total_weight)


# ---------------------------------------------------------------- 6. the two-rank split and the sharded wrapper
@pytest.mark.parametrize("G,N", [(2, 300), (3, 297)])
def test_split_over_two_contexts(G, N):
    import torch
    from sqlp_amd import dist as sdist
    from sqlp_amd import twosd
    M, half, plan = 33, 150, _plan(G)
    ctx, x, data = _context("transship", N)
    vals, w = data[0]
    V = twosd.sdDualVertexSet(ctx)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals, w)
    twosd.solve_push(epi, x, 0, N)
    _, _, ma = twosd._build_cut(epi, x, 0.0, want_argmax=True)
    h = twosd.keep_picks_of_last_cut(epi)
    total = epi.total_scenario_weight
    whole = twosd.reform_cuts(epi, [h], M, SEED, sampling=plan)
    nu, nf = twosd.reform_partial_len(ctx, [h], M)

    def bufs():
        return torch.zeros(nu, dtype=torch.int64, device="cuda"), torch.zeros(nf, dtype=torch.float64, device="cuda")
    u0, f0 = bufs()
    twosd.reform_partial(epi, [h], M, SEED, 0, total, u0.data_ptr(), f0.data_ptr(), sampling=plan)
    ranks = []
    for lo, hi in ((0, half), (half, N)):
        c2, _, _ = _context("transship", N)
        V2 = twosd.sdDualVertexSet(c2)
        V2.push_batch(V.matrix())
        assert V2.fingerprint() == V.fingerprint()
        e2 = twosd.sdEpigraph(c2, 1.0, 0.0)
        twosd.add_scenarios(e2, vals[lo:hi], w[lo:hi])
        _, _, ma2 = twosd._build_cut(e2, x, 0.0, want_argmax=True)
        np.testing.assert_array_equal(ma2, ma[lo:hi])
        h2 = twosd.keep_picks_of_last_cut(e2)
        assert twosd.reform_partial_len(c2, [h2], M) == (nu, nf)
        u, f = bufs()
        twosd.reform_partial(e2, [h2], M, SEED, lo, total, u.data_ptr(), f.data_ptr(), sampling=plan)
        ranks.append((c2, h2, u, f))
    u = ranks[0][2] + ranks[1][2]      # rank order
    f = ranks[0][3] + ranks[1][3]
    torch.cuda.synchronize()
    assert torch.equal(u, u0)          # the integer parts sum exactly
    for c2, h2, _, _ in ranks:
        got = twosd.reform_finalize(c2, [h2], M, total, u.data_ptr(), f.data_ptr())
        np.testing.assert_array_equal(got.weight_mark, whole.weight_mark)
        np.testing.assert_array_equal(got.total_weight, whole.total_weight)
        _close(got.alpha, whole.alpha, "split alpha")
        _close(got.beta, whole.beta, "split beta")
    for c2, _, _, _ in ranks:
        c2.close()
    # one rank: the wrapper makes no collective and is reform_cuts, for the i.i.d. bootstrap and under the plan
    _same_bits(sdist.reform_cuts_sharded(epi, [h], M, SEED, 0, total, sampling=plan), whole)
    _same_bits(sdist.reform_cuts_sharded(epi, [h], M, SEED, 7, total), twosd.reform_cuts(epi, [h], M, SEED, index_offset=7))
    ctx.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    from sqlp_amd import _lib, twosd
    from sqlp_amd._lib import TwoSDError
    ctx, x, data = _context("lands", 302)
    vals = data[0][0]
    V = twosd.sdDualVertexSet(ctx)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals[:101])
    twosd.solve_push(epi, x, 0, 101)
    odd = twosd.build_sasa_cut(epi, x, V, keep_picks=True)                  # N_j = 101
    twosd.add_scenarios(epi, vals[101:300])
    twosd.solve_push(epi, x, 101, 199)
    even = twosd.build_sasa_cut(epi, x, V, keep_picks=True)                 # N_j = 300
    anti = twosd.Sampling.antithetic()

    def refused(text, f, *args, **kw):
        with pytest.raises(TwoSDError) as ei:
            f(*args, **kw)
        assert ei.value.code == -1 and text in str(ei.value), str(ei.value)
    refused("index_offset = 1 is no multiple of the sampling group 2", twosd.reform_cuts, epi, [even], 4, SEED, index_offset=1, sampling=anti)
    refused(f"pick handle {odd.picks} holds 101 scenarios, no multiple of the sampling group 2", twosd.reform_cuts, epi, [even, odd], 4,
            SEED, sampling=anti)
    refused("an LHS plan needs 2 <= group <= 256, not 257", twosd.reform_cuts, epi, [even], 4, SEED, sampling=twosd.Sampling.lhs(257))
    refused("an ANTITHETIC plan has group 2, not 3", twosd.reform_cuts, epi, [even], 4, SEED,
            sampling=twosd.Sampling(_lib.SAMPLING_ANTITHETIC, 3))
    refused("count = 5 is no multiple of the sampling group 2", twosd.bootstrap_counts, ctx, 4, SEED, 0, 5, sampling=anti)
    refused("first_index = 3 is no multiple of the sampling group 2", twosd.bootstrap_counts, ctx, 4, SEED, 3, 6, sampling=anti)
    nu, nf = twosd.reform_partial_len(ctx, [even], 4)
    import torch
    u, f = torch.zeros(nu, dtype=torch.int64, device="cuda"), torch.zeros(nf, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    refused("index_offset = 1 is no multiple", twosd.reform_partial, epi, [even], 4, SEED, 1, 300.0, u.data_ptr(), f.data_ptr(), sampling=anti)
    # a NULL plan and an IID plan through the _vr entries: the old entries, bit for bit
    old = twosd.reform_cuts(epi, [even, odd], 33, SEED, index_offset=1)
    _same_bits(twosd.reform_cuts(epi, [even, odd], 33, SEED, index_offset=1, sampling=twosd.Sampling.iid()), old)
    hs = np.array([even.picks, odd.picks], dtype=np.int32)
    a = np.zeros((34, 2)); b = np.zeros((34, 2, ctx.n1)); wm = np.zeros((34, 2)); tw = np.zeros(34)
    p = lambda arr: arr.ctypes.data_as(C.c_void_p)
    assert ctx.lib.twosd_reform_cuts_vr(ctx.h, epi.index, 2, p(hs), 33, C.c_uint64(SEED), C.c_uint64(1), p(a), p(b), p(wm), p(tw), None) == 0
    _same_bits(twosd.ReformedCuts(a, b, wm, tw), old)
    np.testing.assert_array_equal(twosd.bootstrap_counts(ctx, 5, SEED, 3, 7, sampling=twosd.Sampling.iid()),
                                  twosd.bootstrap_counts(ctx, 5, SEED, 3, 7))
    # an epigraph that holds 301 scenarios
    twosd.add_scenarios(epi, vals[300:301])
    refused(f"epigraph {epi.index} holds 301 scenarios, no multiple of the sampling group 2", twosd.reform_cuts, epi, [even], 4, SEED,
            sampling=anti)
    twosd.add_scenarios(epi, vals[301:302])
    assert twosd.reform_cuts(epi, [even], 4, SEED, sampling=anti).alpha.shape == (5, 1)
    ctx.close()


# ---------------------------------------------------------------- 8. the spread is the stream's
def test_replicate_spread_is_the_antithetic_stream_s():
    """lands at x_EV, 16384 scenarios of stream 777 drawn as antithetic pairs, one cut kept, M = 64.
    v_b = alpha_b + beta_b . x_EV is replicate b's re-formed sample mean of the recourse values (the picks
    were made at this x).  Under the plan its standard deviation over b is the standard error of the pair
    means (band [0.6, 1.6]: a standard deviation on 63 degrees of freedom carries about 9 % relative
    error); resampled as if i.i.d. it is at least 4 times that (DESIGN.md §5.9 measured the two standard
    errors at 0.5653 and 0.0479).  From the C oracle's objectives through the restatement, before any GPU
    run: sd_g 0.04354, sd_s 0.56998, se_g 0.04790, sd_s / sd_g 13.09."""
    from sqlp_amd import smps, twosd
    inst = I.load("lands")
    ctx = twosd.SDContext(inst["sp2"], inst["sto"])
    x = I.x_ev("lands")
    ctx.compute_basis(x, smps.mean_values(inst["sto"]))
    ctx.set_distributions(inst["sto"])
    anti, N, M = twosd.Sampling.antithetic(), 16384, 64
    V = twosd.sdDualVertexSet(ctx)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, N, 777, sampling=anti)
    obj, st, _ = twosd.solve_push(epi, x, 0, N)
    assert (st == 0).all()
    cut = twosd.build_sasa_cut(epi, x, V, tie_rel=0.0, keep_picks=True)
    means, bad = R.grouped(obj, st, 2)
    assert bad == 0 and means.size == N // 2
    se_g = float(means.std(ddof=1) / np.sqrt(means.size))

    def spread(sampling):
        got = twosd.reform_cuts(epi, [cut], M, SEED, sampling=sampling)
        v = got.alpha[:, 0] + got.beta[:, 0] @ x
        assert abs(v[0] - obj.mean()) <= 1e-8 * (1 + abs(obj.mean()))       # the identity row: the sample mean
        return float(v[1:].std(ddof=1))
    sd_g, sd_s = spread(anti), spread(None)
    print(f"sd_g {sd_g:.5f} sd_s {sd_s:.5f} se_g {se_g:.5f} sd_g / se_g {sd_g / se_g:.3f} sd_s / sd_g {sd_s / sd_g:.2f}")
    assert 0.6 * se_g <= sd_g <= 1.6 * se_g
    assert sd_s / sd_g >= 4.0
    ctx.close()


# ---------------------------------------------------------------- 9. end to end
def _run_lands(seed):
    from sqlp_amd import master, smps, twosd
    from tests.test_gpu_sd_loop import _lands_cell
    cell, sp1, sp2 = _lands_cell()
    pos, _, _ = smps.scenario_positions(sp2, I.load("lands")["sto"])
    dists = R.dists_of(I.load("lands")["sto"], pos)
    anti = twosd.Sampling.antithetic()
    it, last = master.sd_run(cell, lambda i: [R.antithetic(dists, 2, 42, first=2 * i)], 30, check_every=10, sampling=anti,
                             stop_args=dict(M=16, seed=seed), quad_scalar_schedule=master.ConstantQuadScalarSchedule(0.1))
    assert it in (10, 20, 30) and last is not None and (last.passed or it == 30)
    assert last.U.shape == last.L.shape == (17,)
    assert cell.epi[0].num_scenarios == 2 * it
    assert last.gaps[0] >= -1e-8 * (1 + abs(last.U[0])), last.gaps[0]
    assert twosd.picks_count(cell.ctx) == len(cell.epi[0].cuts) + 1      # the cuts held and the incumbent cut: no leak
    cell.ctx.close()
    return it, last


def test_sd_run_lands_antithetic_end_to_end():
    """master.sd_run with the default stop under the plan, one antithetic pair per iteration.  The bootstrap
    seed is 8: with some seeds (5 under this plan; 6 and 7 when single scenarios are resampled) the host
    interior-point solver stalls on a replicate's degenerate master and the test raises -- DESIGN.md §9;
    the re-formation is not involved."""
    (ia, a), (ib, b) = _run_lands(8), _run_lands(8)
    assert ia == ib
    np.testing.assert_array_equal(a.U, b.U)
    np.testing.assert_array_equal(a.L, b.L)
    assert a.fraction == b.fraction and a.passed == b.passed
    print(f"lands, antithetic pairs: {ia} iterations, gap {float(a.gaps[0]):.6f}, fraction {a.fraction}")
