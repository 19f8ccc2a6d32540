"""Joint discrete distributions on the device: the block-aware sampler kernels
against the numpy restatement tests/blocks_ref.py (block, DISCRETE and UNIFORM columns bit for bit,
NORMAL within the 1e-12 of tests/test_gpu_sampler.py), the raw entry point with its refusals, and
the consumers of a sampled stream on data/smps/lands3b.

The frequency bound (4 binomial standard errors) and the moments bound (4 of the estimate's own
standard errors) hold for the reference streams at the seeds used here, computed on the CPU from
blocks_ref and the six recourse values before the seeds were fixed: realisation frequencies
|z| <= 1.72 (IID), 2.05 (ANTITHETIC), 0.81 (LHS 16); evaluate_moments at seed 4242, N = 32768
z = -0.10 (IID), 0.61 (ANTITHETIC), 0.49 (LHS 16)."""
import functools
import os

import numpy as np
import pytest

from tests import blocks_ref as B
from tests import instances as I
from tests import vr_ref as V

pytestmark = pytest.mark.gpu

DATA = I.DATA
# recourse values of the six realisations of lands3b at lands' x_EV (HiGHS, four decimals), their
# exact expectation and standard deviation
HIGHS_OBJ = [174.4, 258.6667, 360.6667, 236.1667, 237.7, 259.6667]
EXACT_RECOURSE, RECOURSE_SD = 253.781667, 52.62


def _sampling(plan):
    from sqlp_amd import twosd
    if plan == "iid":
        return None
    return twosd.Sampling.antithetic() if plan == "antithetic" else twosd.Sampling.lhs(plan[1])


def _group(plan):
    return 1 if plan == "iid" else 2 if plan == "antithetic" else plan[1]


def _draw(ctx, N, seed, first, plan):
    from sqlp_amd import twosd
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, N, seed, first_index=first, sampling=_sampling(plan))
    assert epi.num_scenarios == N
    return twosd.get_scenarios(epi)


def _match(ctx, got, ref, dists):
    """An epigraph stores value - template and get_scenarios adds the template back: the reference
    values take the same two roundings (as in tests/test_gpu_vr.py)."""
    ref = (ref - ctx.template_values) + ctx.template_values
    exact = np.array([d[0] != "NORMAL" for d in dists])
    np.testing.assert_array_equal(got[:, exact], ref[:, exact])
    if (~exact).any():
        print(f"NORMAL columns: max abs error {np.abs(got[:, ~exact] - ref[:, ~exact]).max():.3e}")
        np.testing.assert_allclose(got[:, ~exact], ref[:, ~exact], rtol=1e-12, atol=1e-12)


# ---- 1. parity on lands3b ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lands3b():
    from sqlp_amd import smps, twosd
    cor, tim, sto = smps.load_smps(os.path.join(DATA, "lands3b"))
    sp2 = smps.get_smps_stage_template(cor, tim, 2)
    ctx = twosd.SDContext(sp2, sto)
    ctx.set_distributions(sto)
    dists, blocks = B.table_of(sto, ctx.positions)
    support, probs = smps.joint_support(sto, ctx.positions)
    return dict(cor=cor, tim=tim, sto=sto, sp2=sp2, ctx=ctx, dists=dists, blocks=blocks, support=support, probs=probs)


@pytest.mark.parametrize("plan,first", [("iid", 7), ("antithetic", 8), (("lhs", 16), 16)])
def test_lands3b_stream_parity(plan, first):
    L = _lands3b()
    ctx = L["ctx"]
    N, seed = 20000, 0x5EED1234ABCDEF
    assert ctx.k == 3 and first % _group(plan) == 0 and N % _group(plan) == 0
    got = _draw(ctx, N, seed, first, plan)
    ref = B.draw(plan, L["dists"], L["blocks"], N, seed, first)
    np.testing.assert_array_equal(got, ref)
    # every row is one of the six realisations, at the stated frequencies
    hit = (got[:, None, :] == L["support"][None, :, :]).all(axis=2)
    assert (hit.sum(axis=1) == 1).all()
    p = L["probs"]
    z = (hit.mean(axis=0) - p) / np.sqrt(p * (1 - p) / N)
    print(f"{plan}: realisation frequency z = {np.round(z, 2)}")
    assert np.abs(z).max() <= 4.0


# ---- 2. a mixed table: the three kinds, three blocks, the counter carry --------------------------------
@functools.lru_cache(maxsize=None)
def _mixed():
    """Template "g" (k = 16) in its own layout order, so that the blocks' members lie between the
    independent elements: block A = elements [10, 3, 5] (lead 10) with R = 1000, zero-probability
    runs (leading, inside, trailing) and total mass 0.9; block B = [6] with unsorted, repeated
    values; block C = [12, 9] with R = 1."""
    from sqlp_amd import twosd
    from sqlp_amd.smps import spSmpsPosition, spStoBlock, spStoType
    from tests import synth_cases as SC
    S = SC.template("g")
    pos = [spSmpsPosition(*p) for p in S.positions]
    assert len(pos) == 16
    indep = {0: ("DISCRETE", [1.0, 4.0, 2.0], [0.3, 0.3, 0.3]), 1: ("NORMAL", 10.0, 4.0), 2: ("UNIFORM", -1.0, 3.0),
             4: ("DISCRETE", [2.5], [1.0]), 7: ("UNIFORM", 100.0, 100.5), 8: ("NORMAL", -3.0, 0.25),
             11: ("DISCRETE", [7.0, 3.0, 5.0], [0.3, 0.3, 0.4]), 13: ("NORMAL", 0.5, 1.0), 14: ("DISCRETE", [-1.0, 1.0], [0.5, 0.5]),
             15: ("UNIFORM", 0.0, 1.0)}
    rng = np.random.default_rng(20240)
    R = 1000
    p = rng.uniform(0.05, 1.0, size=R)
    p[:7] = 0.0
    p[400:460] = 0.0
    p[700] = 0.0
    p[-25:] = 0.0
    p *= 0.9 / p.sum()
    va = np.round(rng.normal(0.0, 3.0, size=(R, 3)), 6)
    sto = spStoType("synthetic", {pos[e]: d for e, d in indep.items()})
    sto.blocks = [spStoBlock("A", "P2", [pos[10], pos[3], pos[5]], p.tolist(), va.tolist()),
                  spStoBlock("B", "P2", [pos[6]], [0.25, 0.25, 0.25, 0.25], [[3.0], [1.0], [2.0], [1.0]]),
                  spStoBlock("C", "P2", [pos[12], pos[9]], [0.5], [[1.5, -2.5]])]
    ctx = twosd.SDContext(S.sp2, sto, positions=pos)
    ctx.set_distributions(sto)
    dists, blocks = B.table_of(sto, ctx.positions)
    assert [b[0] for b in blocks] == [[10, 3, 5], [6], [12, 9]]
    assert {d[0] for d in dists} == {"DISCRETE", "NORMAL", "UNIFORM", "BLOCK"}
    return ctx, dists, blocks


@pytest.mark.parametrize("plan", ["iid", "antithetic", ("lhs", 5)])
def test_mixed_table_and_counter_carry(plan):
    ctx, dists, blocks = _mixed()
    G = _group(plan)
    N, seed, first = 1000, 0x9E3779B97F4A7C15, 2 ** 32 - 300
    first -= first % G                     # LHS: on the group boundary below
    assert (N * ctx.k) % 256 and seed >> 32 and first < 2 ** 32 < first + N
    got = _draw(ctx, N, seed, first, plan)
    ref = B.draw(plan, dists, blocks, N, seed, first)
    _match(ctx, got, ref, dists)
    # the reference has what the case is about: block A reaches its last realisation past its mass
    # (a tenth of the draws), never a zero-probability one before it; B keeps its repeated value;
    # the high counter word matters
    pa, va = np.asarray(blocks[0][1]), blocks[0][2]
    ia = B.walk(pa, np.array([0.0, 0.95]))
    assert pa[ia[0]] > 0 and ia[0] == 7 and ia[1] == len(pa) - 1
    last = (ref[:, [10, 3, 5]] == va[-1]).all(axis=1).mean()
    assert 0.05 < last < 0.16
    assert 0.4 < (ref[:, 6] == 1.0).mean() < 0.6
    assert (ref[:, 12] == 1.5).all() and (ref[:, 9] == -2.5).all()
    low = B.draw(plan, dists, blocks, N, seed, first + 10 * 2 ** 32)      # the same low words, other high ones
    assert (low[:, [10, 3, 5]] != ref[:, [10, 3, 5]]).any()
    # two shards split at the 2^32 carry (LHS: at the first group boundary at or past it, the group
    # that straddles the carry staying whole) reproduce the single draw
    from sqlp_amd import twosd
    n1 = -(-(2 ** 32 - first) // G) * G
    two = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(two, n1, seed, first_index=first, sampling=_sampling(plan))
    twosd.add_sampled_scenarios(two, N - n1, seed, first_index=first + n1, sampling=_sampling(plan))
    np.testing.assert_array_equal(twosd.get_scenarios(two), got)


# ---- 3. the raw entry point: permuted members, refusals, dropping the blocks ---------------------------
def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _joint(ctx, kind, nsup, vals, probs, p0, p1, moff, mem, nreal, bp, bv):
    from sqlp_amd._lib import ptr
    a = [_i32(kind), _i32(nsup), _f64(vals), _f64(probs), _f64(p0), _f64(p1)]
    b = [_i32(moff), _i32(mem), _i32(nreal), _f64(bp), _f64(bv)]
    return ctx.lib.twosd_set_distributions_joint(ctx.h, len(kind), *[ptr(v) for v in a], len(nreal), *[ptr(v) for v in b])


def test_raw_abi_permuted_members_and_refusals():
    from sqlp_amd import twosd
    from sqlp_amd._lib import ptr
    from sqlp_amd.smps import spSmpsPosition, spStoType
    from tests import synth_cases as SC
    S = SC.template("e")
    pos = [spSmpsPosition(*p) for p in S.positions]
    assert len(pos) == 8
    ctx = twosd.SDContext(S.sp2, None, positions=pos)
    disc0, disc5 = ("DISCRETE", [1.0, 4.0, 2.0], [0.3, 0.3, 0.3]), ("DISCRETE", [-1.0, 1.0], [0.5, 0.5])
    dists = [disc0, ("BLOCK",), ("NORMAL", 10.0, 4.0), ("UNIFORM", -1.0, 3.0), ("BLOCK",), disc5, ("BLOCK",), ("UNIFORM", 0.0, 2.0)]
    bp = [0.2, 0.0, 0.5, 0.3]
    bv = np.array([[40.0, 10.0, 60.0], [41.0, 11.0, 61.0], [42.0, 12.0, 62.0], [43.0, 13.0, 63.0]])   # columns: elements 4, 1, 6
    blocks = [([4, 1, 6], bp, bv)]
    good = dict(kind=[0, 3, 1, 2, 3, 0, 3, 2], nsup=[3, 0, 0, 0, 0, 2, 0, 0], vals=disc0[1] + disc5[1], probs=disc0[2] + disc5[2],
                p0=[0, 0, 10.0, -1.0, 0, 0, 0, 0.0], p1=[0, 0, 4.0, 3.0, 0, 0, 0, 2.0],
                moff=[0, 3], mem=[4, 1, 6], nreal=[4], bp=bp, bv=bv.ravel())
    assert _joint(ctx, **good) == 0
    N, seed, first = 256, 31337, 5
    got = _draw(ctx, N, seed, first, "iid")
    ref = B.iid(dists, blocks, N, seed, first)
    _match(ctx, got, ref, dists)
    assert set(np.unique(ref[:, 4])) == {40.0, 42.0, 43.0}                  # the lead's column; p = 0 never drawn
    np.testing.assert_array_equal(ref[:, 1], ref[:, 4] - 30.0)
    np.testing.assert_array_equal(ref[:, 6], ref[:, 4] + 20.0)
    _match(ctx, _draw(ctx, N, seed, 8, ("lhs", 8)), B.lhs(dists, blocks, 8, N, seed, 8), dists)

    nan, inf = float("nan"), float("inf")
    bad_value = bv.copy().ravel()
    refusals = {
        "kind 3 in no block": dict(kind=[3, 3, 1, 2, 3, 0, 3, 2], nsup=[0, 0, 0, 0, 0, 2, 0, 0], vals=disc5[1], probs=disc5[2]),
        "in two blocks": dict(moff=[0, 3, 4], mem=[4, 1, 6, 1], nreal=[4, 1], bp=bp + [1.0], bv=list(bv.ravel()) + [0.0]),
        "twice in one": dict(mem=[4, 1, 4]),
        "member kind": dict(mem=[4, 1, 0]),
        "nreal 0": dict(nreal=[0]),
        "empty block": dict(moff=[0, 3, 3], nreal=[4, 1], bp=bp + [1.0]),
        "negative probability": dict(bp=[0.2, -0.1, 0.5, 0.3]),
        "nan probability": dict(bp=[0.2, nan, 0.5, 0.3]),
        "inf probability": dict(bp=[0.2, inf, 0.5, 0.3]),
        "nan value": dict(bv=np.where(np.arange(12) == 7, nan, bad_value)),
        "inf value": dict(bv=np.where(np.arange(12) == 11, -inf, bad_value)),
        "member below 0": dict(mem=[4, -1, 6]),
        "member past k": dict(mem=[4, 8, 6]),
    }
    for name, change in refusals.items():
        assert _joint(ctx, **{**good, **change}) == -1, name
        assert b"set_distributions" in ctx.lib.twosd_last_error(), name
    # past the 32-bit table offsets: refused from the shapes alone, before any table is read
    assert _joint(ctx, **{**good, "nreal": [2 ** 31 - 1]}) == -5
    # ... and the previous tables are still in use
    np.testing.assert_array_equal(_draw(ctx, N, seed, first, "iid"), got)
    # the plain entry point still refuses kind 3
    plain = [_i32(good["kind"]), _i32(good["nsup"]), _f64(good["vals"]), _f64(good["probs"]), _f64(good["p0"]), _f64(good["p1"])]
    assert ctx.lib.twosd_set_distributions(ctx.h, 8, *[ptr(v) for v in plain]) == -1
    assert b"unknown kind 3" in ctx.lib.twosd_last_error()
    np.testing.assert_array_equal(_draw(ctx, N, seed, first, "iid"), got)
    # nblocks == 0 is the plain call, which drops the blocks: the stream is vr_ref's
    indep = [disc0, disc5, ("NORMAL", 10.0, 4.0), ("UNIFORM", -1.0, 3.0), disc5, disc5, disc0, ("UNIFORM", 0.0, 2.0)]
    sto = spStoType("plain", dict(zip(pos, indep)))
    ctx.set_distributions(sto)
    after = _draw(ctx, N, seed, first, "iid")
    _match(ctx, after, V.iid(indep, N, seed, first), indep)
    kinds = [{"DISCRETE": 0, "NORMAL": 1, "UNIFORM": 2}[d[0]] for d in indep]
    nsup = [len(d[1]) if d[0] == "DISCRETE" else 0 for d in indep]
    vals = [v for d in indep if d[0] == "DISCRETE" for v in d[1]]
    probs = [v for d in indep if d[0] == "DISCRETE" for v in d[2]]
    p0 = [0.0 if d[0] == "DISCRETE" else d[1] for d in indep]
    p1 = [0.0 if d[0] == "DISCRETE" else d[2] for d in indep]
    assert _joint(ctx, **good) == 0
    assert _joint(ctx, kinds, nsup, vals, probs, p0, p1, [0], [], [], [], []) == 0
    np.testing.assert_array_equal(_draw(ctx, N, seed, first, "iid"), after)


# ---- 4. a one-member ascending block is the INDEP DISCRETE stream ---------------------------------------
@pytest.mark.parametrize("plan", ["iid", "antithetic", ("lhs", 8)])
def test_one_member_block_equals_indep_discrete(plan):
    from sqlp_amd import twosd
    from sqlp_amd.smps import spSmpsPosition, spStoBlock, spStoType
    from tests import synth_cases as SC
    S = SC.template("e")
    pos = [spSmpsPosition(*p) for p in S.positions]
    disc = ("DISCRETE", [-2.0, 0.5, 3.0, 7.0], [0.2, 0.0, 0.3, 0.4])          # ascending, mass 0.9, a zero
    indep = [("DISCRETE", [1.0, 4.0, 2.0], [0.3, 0.3, 0.3]), ("NORMAL", 10.0, 4.0), ("UNIFORM", -1.0, 3.0), ("DISCRETE", [2.5], [1.0]),
             disc, ("UNIFORM", 100.0, 100.5), ("NORMAL", -3.0, 0.25), ("DISCRETE", [-1.0, 1.0], [0.5, 0.5])]
    a = spStoType("indep", dict(zip(pos, indep)))
    b = spStoType("block", {p: d for e, (p, d) in enumerate(zip(pos, indep)) if e != 4})
    b.blocks = [spStoBlock("ONE", "P2", [pos[4]], list(disc[2]), [[v] for v in disc[1]])]
    out = []
    for sto in (a, b):
        ctx = twosd.SDContext(S.sp2, sto, positions=pos)
        ctx.set_distributions(sto)
        out.append(_draw(ctx, 1024, 0x9E3779B97F4A7C15, 2 ** 32 - 512, plan))
    np.testing.assert_array_equal(out[1], out[0])
    assert len(np.unique(out[0][:, 4])) == 3


# ---- 5. the consumers on lands3b at x_EV ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lands3b_solved():
    """lands3b's context with the basis of x_EV, the first-stage cost, and the six recourse values
    with their exact expectation."""
    from oracle import lp_highs
    from sqlp_amd import smps
    L = _lands3b()
    ctx, sto = L["ctx"], L["sto"]
    x = I.x_ev("lands")
    ctx.compute_basis(x, smps.mean_values(sto))
    c1 = smps.get_smps_stage_template(L["cor"], L["tim"], 1).q
    obj, _, _, st = ctx.solve_values(x, L["support"], want_pi=False)
    assert (st == 0).all()
    # the same six LPs through HiGHS on the oracle's template of lands (the same core file)
    sp = I.load("lands")["osp2"]
    hi = []
    for v in L["support"]:
        b = sp.r - sp.T @ x
        b[ctx.rows] += v - sp.r[ctx.rows]
        status, o, _, _ = lp_highs.solve_rhs(sp, b)
        assert status == 0
        hi.append(o)
    np.testing.assert_allclose(obj, hi, rtol=1e-9)
    np.testing.assert_allclose(hi, HIGHS_OBJ, rtol=0, atol=5e-5)
    exact = float(L["probs"] @ obj)
    assert abs(exact - EXACT_RECOURSE) <= 1e-6 and abs(np.sqrt(L["probs"] @ (obj - exact) ** 2) - RECOURSE_SD) <= 5e-3
    return ctx, x, c1, obj, exact


def test_sampled_epigraph_solves_like_its_values():
    from sqlp_amd import twosd
    ctx, x, _, obj6, _ = _lands3b_solved()
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, 2048, 99, first_index=64, sampling=twosd.Sampling.lhs(64))
    o_e, _, _, st_e = twosd.solve_batch(epi, x, want_pi=False)
    o_v, _, _, st_v = ctx.solve_values(x, twosd.get_scenarios(epi), want_pi=False)
    assert (st_e == 0).all() and (st_v == 0).all()
    np.testing.assert_allclose(o_e, o_v, rtol=1e-12)
    assert len(np.unique(np.round(o_e, 6))) == 6
    assert np.abs(o_e[:, None] - obj6[None, :]).min(axis=1).max() <= 1e-9 * 400


@pytest.mark.parametrize("plan", ["iid", "antithetic", ("lhs", 16)])
def test_evaluate_moments_covers_the_exact_expectation(plan):
    from sqlp_amd import twosd
    ctx, x, c1, _, exact = _lands3b_solved()
    m = twosd.evaluate_moments(ctx, c1, x, 4242, 0, 32768, sampling=_sampling(plan))
    want = float(np.dot(c1, x)) + exact
    assert m.n_bad == 0 and m.n_scenarios == 32768 and m.group == _group(plan)
    z = (m.mean - want) / m.std_error
    print(f"{plan}: mean {m.mean:.6f}, exact {want:.6f}, standard error {m.std_error:.4f}, z = {z:.2f}")
    assert abs(z) <= 4.0


def test_evaluate_sampled_shards_add_up():
    from sqlp_amd import twosd
    ctx, x, c1, _, exact = _lands3b_solved()
    N, seed = 30000, 4242
    val = twosd.evaluate_sampled(ctx, c1, x, N, seed)
    h = N // 3
    zero = np.zeros(len(x))
    s_a = twosd.evaluate_sampled(ctx, zero, x, N, seed, 0, h)
    s_b = twosd.evaluate_sampled(ctx, zero, x, N, seed, h, N - h)
    assert abs(float(np.dot(c1, x)) + s_a + s_b - val) <= 1e-10 * (1 + abs(val))
    assert abs(val - float(np.dot(c1, x)) - exact) <= 4 * RECOURSE_SD / np.sqrt(N) + 1e-3     # z = -0.1 at 32768: the same stream


def test_pool_refresh_on_a_block_stream():
    """A pool built and refreshed from sampled scenarios of lands3b (the selection key's spread comes
    from the members' marginals): every solve stays optimal and equals the no-pool solve."""
    from sqlp_amd import smps, twosd
    L = _lands3b()
    sto, sp2 = L["sto"], L["sp2"]
    x_ev = I.x_ev("lands")
    x2 = x_ev * 1.07 + 0.01
    ctx = twosd.SDContext(sp2, sto)
    ctx.set_distributions(sto)
    ctx.compute_basis(x_ev, smps.mean_values(sto))
    tr = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(tr, 512, 32)
    ctx.pool_build(tr, x_ev, 0, 512, 32)
    ev = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(ev, 2000, 31)
    P = ctx.pool_refresh(tr, x2, 0, 512, 32)
    assert 1 <= P <= 32
    o, _, _, st = twosd.solve_batch(ev, x2, 0, 2000, want_pi=False)
    ref = twosd.SDContext(sp2, sto)                                 # primary basis only
    ref.compute_basis(x_ev, smps.mean_values(sto))
    o_ref, _, _, st_ref = ref.solve_values(x2, twosd.get_scenarios(ev), want_pi=False)
    assert (st == 0).all() and (st_ref == 0).all()
    np.testing.assert_allclose(o, o_ref, rtol=1e-9)
    print(f"lands3b: pool {P}, pivots {ctx.lp_stats()[0] / 2000:.2f}")
