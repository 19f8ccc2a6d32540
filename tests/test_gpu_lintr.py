"""Correlated continuous elements on the device (SMPS BLOCKS LINTR): the latent
pass and lintr_apply_kernel against the numpy restatement tests/lintr_ref.py (bit for bit where
no latent is NORMAL), chunking and sharding, the raw entry point with its refusals, mvnormal_lintr,
and the consumers of a sampled stream on data/smps/lands3t.

Reference-only conditions, checked on the CPU before the seeds were fixed: the restated
mvnormal_lintr stream at seed 20261021, N = 65536 has every sample covariance entry within 6
standard errors of cov (largest |z| = 2.31); the lands3t streams are those of
tests/test_lintr_host.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lintr_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = ["iid", "antithetic", ("lhs", 16)]
N_SMALL, SEED, FIRST = 96, 0x9E3779B97F4A7C15, 2 ** 32 - 32         # the counter carry inside the draw
MVN_SEED, MVN_N = 20261021, 65536


def plan_name(plan):
    return plan if isinstance(plan, str) else f"lhs{plan[1]}"


def _sampling(plan):
    from sqlp_amd import twosd
    if plan == "iid":
        return None
    return twosd.Sampling.antithetic() if plan == "antithetic" else twosd.Sampling.lhs(plan[1])


def draw(ctx, N, seed, first, plan, parts=1):
    from sqlp_amd import twosd
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    for i in range(parts):
        twosd.add_sampled_scenarios(epi, N // parts, seed, first_index=first + i * (N // parts), sampling=_sampling(plan))
    assert epi.num_scenarios == N
    return twosd.get_scenarios(epi)


def _stored(ctx, ref):
    """An epigraph stores value - template and get_scenarios adds the template back: the reference
    values take the same two roundings (as in tests/test_gpu_vr.py)."""
    return (ref - ctx.template_values) + ctx.template_values


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the small mixed layout -----------------------------------------------------------------------------
LATENTS = {
    "exact": [("DISCRETE", [2.0, -1.0, 0.5], [0.3, 0.3, 0.3]), ("UNIFORM", -1.0, 3.0)],
    "normal": [("NORMAL", 1.0, 4.0), ("NORMAL", -0.5, 0.25)],
}


@functools.lru_cache(maxsize=None)
def _template():
    from sqlp_amd.smps import spSmpsPosition
    from tests import synth_cases as SC
    S = SC.synth_template(20, 129, 6, 31, amp=0.7)
    return S, [spSmpsPosition(*p) for p in S.positions]


def small_sto(which, second=False, lintr=True):
    """k = 6: element 1 INDEP UNIFORM, a two-member discrete block [4, 2], a LINTR block with members
    [5, 0, 3], q = 2 and rows of 2, 1 and 0 entries.  second: element 1 is a LINTR block of its own
    (n = 1, q = 1) after the first.  lintr=False: the LINTR members are INDEP UNIFORM elements."""
    from sqlp_amd.smps import spStoBlock, spStoLintr, spStoType
    _, pos = _template()
    sto = spStoType("synthetic", {} if second else {pos[1]: ("UNIFORM", 10.0, 12.0)})
    sto.blocks = [spStoBlock("D", "P2", [pos[4], pos[2]], [0.25, 0.5, 0.25], [[1.0, -1.0], [2.0, -2.0], [3.0, -3.0]])]
    if not lintr:
        for e in (5, 0, 3):
            sto.indep[pos[e]] = ("UNIFORM", 0.0, 1.0)
        return sto
    sto.lintr = [spStoLintr("L", "P2", [pos[5], pos[0], pos[3]], [10.1, -2.3, 0.75], ["A", "B"], list(LATENTS[which]),
                            [[(0, 1.3), (1, -0.7)], [(1, 2.1)], []])]
    if second:
        sto.lintr.append(spStoLintr("L2", "P2", [pos[1]], [4.0], ["C"], [("UNIFORM", 0.0, 8.0)], [[(0, 0.3)]]))
    return sto


def small(which, second=False, lintr=True):
    from sqlp_amd import twosd
    S, pos = _template()
    sto = small_sto(which, second, lintr)
    ctx = twosd.SDContext(S.sp2, sto, positions=pos)
    ctx.set_distributions(sto)
    return ctx, R.table_of(sto, ctx.positions) if lintr else None


def test_library_exports_the_entry_point():
    from sqlp_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "twosd_set_distributions_lintr")
    assert lib.twosd_set_distributions_lintr.argtypes is not None and len(lib.twosd_set_distributions_lintr.argtypes) == 15


@pytest.mark.parametrize("plan", PLANS, ids=plan_name)
def test_stream_parity_bit_for_bit(plan):
    ctx, (dists, blocks, lintr) = small("exact")
    assert ctx.k == 6 and lintr[0][0] == [5, 0, 3] and [len(r) for r in lintr[0][3]] == [2, 1, 0] and blocks[0][0] == [4, 2]
    got = draw(ctx, N_SMALL, SEED, FIRST, plan)
    ref = _stored(ctx, R.draw(plan, dists, blocks, lintr, N_SMALL, SEED, FIRST))
    np.testing.assert_array_equal(_bits(got), _bits(ref))
    # the case can tell a fused multiply-add from the contract's two roundings: for some scenario the
    # fused member differs from the restated one
    xi = R.latents(plan, 6, lintr, N_SMALL, SEED, FIRST)
    fused = np.array([float(np.longdouble(2.1) * np.longdouble(u) + np.longdouble(-2.3)) for u in xi[:, 1]])
    assert (fused != -2.3 + 2.1 * xi[:, 1]).any()
    assert len(np.unique(got[:, 5])) > 90 and (np.unique(got[:, 3]) == _stored(ctx, np.full((1, 6), 0.75))[0, 3]).all()
    # the other columns are those of the same context with the members replaced by INDEP elements
    plain = small_sto("exact", lintr=False)
    ctx.set_distributions(plain)
    np.testing.assert_array_equal(_bits(draw(ctx, N_SMALL, SEED, FIRST, plan)[:, [1, 2, 4]]), _bits(got[:, [1, 2, 4]]))
    ctx.close()


@pytest.mark.parametrize("plan", PLANS, ids=plan_name)
def test_stream_parity_normal_latents(plan):
    ctx, (dists, blocks, lintr) = small("normal")
    got = draw(ctx, N_SMALL, SEED, FIRST, plan)
    ref = _stored(ctx, R.draw(plan, dists, blocks, lintr, N_SMALL, SEED, FIRST))
    np.testing.assert_array_equal(_bits(got[:, [1, 2, 4]]), _bits(ref[:, [1, 2, 4]]))
    # 1e-12 (|c| + sum |h| (|mean| + sd max(1, |z|))): the project's NORMAL bound through the sum
    xi = R.latents(plan, 6, lintr, N_SMALL, SEED, FIRST)
    members, constants, lat, rows = lintr[0]
    for j, e in enumerate(members):
        bound = np.full(N_SMALL, abs(constants[j]))
        for l, h in rows[j]:
            mean, sd = lat[l][1], np.sqrt(lat[l][2])
            bound = bound + abs(h) * (abs(mean) + sd * np.maximum(1.0, np.abs((xi[:, l] - mean) / sd)))
        err = np.abs(got[:, e] - ref[:, e])
        print(f"{plan_name(plan)}: member {e}: max error {err.max():.3e}, smallest bound {1e-12 * bound.min():.3e}")
        assert (err <= 1e-12 * bound).all()
    ctx.close()


def test_chunking_in_a_fresh_process(tmp_path):
    """TWOSD_LINTR_CHUNK=32 (three chunks of 32; LHS 16: two groups each; new allocations poisoned)
    gives the bits of the default, one-chunk draw."""
    env = dict(os.environ, TWOSD_LINTR_CHUNK="32", TWOSD_POISON="255", TWOSD_POISON_FAMILY="7")
    out = tmp_path / "chunked.npz"
    r = subprocess.run([sys.executable, "-m", "tests.lintr_child", str(out)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, f"child failed ({r.returncode}):\n{r.stderr[-3000:]}"
    chunked = np.load(out)
    assert "TWOSD_LINTR_CHUNK" not in os.environ
    ctx, _ = small("exact")
    for plan in PLANS:
        np.testing.assert_array_equal(_bits(chunked[plan_name(plan)]), _bits(draw(ctx, N_SMALL, SEED, FIRST, plan)))
    ctx.close()


@pytest.mark.parametrize("plan", PLANS, ids=plan_name)
def test_two_calls_of_48_equal_one_of_96(plan):
    ctx, _ = small("exact")
    np.testing.assert_array_equal(_bits(draw(ctx, N_SMALL, SEED, FIRST, plan, parts=2)), _bits(draw(ctx, N_SMALL, SEED, FIRST, plan)))
    ctx.close()


@pytest.mark.parametrize("plan", PLANS, ids=plan_name)
def test_second_block_numbers_its_latent_globally(plan):
    ctx, (dists, blocks, lintr) = small("exact", second=True)
    assert [b[0] for b in lintr] == [[5, 0, 3], [1]] and sum(len(b[2]) for b in lintr) == 3
    got = draw(ctx, N_SMALL, SEED, FIRST, plan)
    ref = _stored(ctx, R.draw(plan, dists, blocks, lintr, N_SMALL, SEED, FIRST))
    np.testing.assert_array_equal(_bits(got), _bits(ref))
    # element 1 is 4 + 0.3 * (latent 2 = element word k + 2), not the block's own latent 0
    xi = R.latents(plan, 6, lintr, N_SMALL, SEED, FIRST)
    np.testing.assert_array_equal(ref[:, 1], _stored(ctx, np.tile(4.0 + 0.3 * xi[:, 2:3], (1, 6)))[:, 1])
    assert (xi[:, 2] != xi[:, 0]).any() and len(np.unique(xi[:, 2])) > 90
    ctx.close()


def test_antithetic_pairs_of_a_uniform_block():
    """Even + odd member of a pair = 2 c + H (left + right), to 4 ulp of the largest term."""
    from sqlp_amd import twosd
    from sqlp_amd.smps import spStoLintr, spStoType
    S, pos = _template()
    lat = [("UNIFORM", -1.0, 3.0), ("UNIFORM", 0.0, 8.0)]
    c, rows = [100.0, -200.0, 50.0], [[(0, 1.5), (1, -0.5)], [(1, 2.0)], [(0, 4.0)]]
    sto = spStoType("synthetic", {pos[e]: ("UNIFORM", 0.0, 1.0) for e in (1, 2, 4)})
    sto.lintr = [spStoLintr("L", "P2", [pos[5], pos[0], pos[3]], c, ["A", "B"], lat, rows)]
    ctx = twosd.SDContext(S.sp2, sto, positions=pos)
    ctx.set_distributions(sto)
    got = draw(ctx, N_SMALL, SEED, FIRST, "antithetic")
    for j, e in enumerate([5, 0, 3]):
        terms = [2 * c[j]] + [h * (lat[l][1] + lat[l][2]) for l, h in rows[j]]
        pair = got[0::2, e] + got[1::2, e]
        err = np.abs(pair - sum(terms)).max()
        print(f"member {e}: pair sums off by at most {err:.3e}, 4 ulp = {4 * np.spacing(max(abs(t) for t in terms)):.3e}")
        assert err <= 4 * np.spacing(max(abs(t) for t in terms))
        assert len(np.unique(got[:, e])) > 90
    ctx.close()


# ---- the raw entry point ----------------------------------------------------------------------------------
def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


GOOD = dict(kind=[4, 2, 3, 4, 3, 4], nsup=[0] * 6, vals=[0.0], probs=[0.0], p0=[0, 10.0, 0, 0, 0, 0], p1=[0, 12.0, 0, 0, 0, 0],
            moff=[0, 2], mem=[4, 2], nreal=[3], bp=[0.25, 0.5, 0.25], bv=[1.0, -1.0, 2.0, -2.0, 3.0, -3.0],
            lmoff=[0, 3], lmem=[5, 0, 3], lc=[10.1, -2.3, 0.75], loff=[0, 2], lkind=[0, 2], lnsup=[3, 0], lvals=[2.0, -1.0, 0.5],
            lprobs=[0.3, 0.3, 0.3], lp0=[0.0, -1.0], lp1=[0.0, 3.0], rptr=[0, 2, 3, 3], col=[0, 1, 1], val=[1.3, -0.7, 2.1])


def _raw(ctx, kind, nsup, vals, probs, p0, p1, moff, mem, nreal, bp, bv, lmoff, lmem, lc, loff, lkind, lnsup, lvals, lprobs, lp0, lp1,
         rptr, col, val, nlintr=None):
    import ctypes as C
    from sqlp_amd import _lib
    from sqlp_amd._lib import ptr
    a = [_i32(kind), _i32(nsup), _f64(vals), _f64(probs), _f64(p0), _f64(p1)]
    b = [_i32(moff), _i32(mem), _i32(nreal), _f64(bp), _f64(bv)]
    keep = [_i32(lmoff), _i32(lmem), _f64(lc), _i32(loff), _i32(lkind), _i32(lnsup), _f64(lvals), _f64(lprobs), _f64(lp0), _f64(lp1),
            _i32(rptr), _i32(col), _f64(val)]
    L = _lib.Lintr(len(loff) - 1 if nlintr is None else nlintr, *[ptr(v) for v in keep])
    return ctx.lib.twosd_set_distributions_lintr(ctx.h, len(kind), *[ptr(v) for v in a], len(nreal), *[ptr(v) for v in b], C.byref(L))


def test_raw_abi_refusals_and_dropping_the_tables():
    from sqlp_amd import twosd
    from sqlp_amd._lib import ptr
    S, pos = _template()
    ctx = twosd.SDContext(S.sp2, None, positions=pos)
    assert _raw(ctx, **GOOD) == 0
    dists, blocks, lintr = R.table_of(small_sto("exact"), ctx.positions)
    got = draw(ctx, N_SMALL, SEED, FIRST, "iid")
    np.testing.assert_array_equal(_bits(got), _bits(_stored(ctx, R.draw("iid", dists, blocks, lintr, N_SMALL, SEED, FIRST))))
    nan, inf = float("nan"), float("inf")
    refusals = {
        "kind 4 in no block": (dict(kind=[4, 4, 3, 4, 3, 4], p0=[0] * 6, p1=[0] * 6), b"element 1"),
        "in two blocks": (dict(lmoff=[0, 3, 4], lmem=[5, 0, 3, 0], lc=[10.1, -2.3, 0.75, 1.0], loff=[0, 2, 3], lkind=[0, 2, 2],
                               lnsup=[3, 0, 0], lp0=[0, -1.0, 0], lp1=[0, 3.0, 1], rptr=[0, 2, 3, 3, 4], col=[0, 1, 1, 0],
                               val=[1.3, -0.7, 2.1, 1.0]), b"LINTR block 1"),
        "twice in one": (dict(lmem=[5, 0, 5]), b"LINTR block 0"),
        "member kind": (dict(lmem=[5, 1, 3]), b"kind is not 4"),
        "member past k": (dict(lmem=[5, 6, 3]), b"outside [0, k)"),
        "empty block": (dict(lmoff=[0, 3, 3], loff=[0, 2, 3]), b"without members"),
        "no latent": (dict(loff=[0, 0]), b"fewer than one latent"),
        "column past q": (dict(col=[0, 2, 1]), b"CSR column"),
        "column below 0": (dict(col=[-1, 1, 1]), b"CSR column"),
        "columns not ascending": (dict(col=[1, 0, 1]), b"CSR column"),
        "columns repeated": (dict(col=[1, 1, 1]), b"CSR column"),
        "nan constant": (dict(lc=[10.1, nan, 0.75]), b"non-finite constant"),
        "inf coefficient": (dict(val=[1.3, -inf, 2.1]), b"non-finite coefficient"),
        "latent kind": (dict(lkind=[0, 3]), b"latent 1"),
        "latent empty support": (dict(lnsup=[0, 0]), b"latent 0"),
        "latent repeated support": (dict(lvals=[2.0, -1.0, 2.0]), b"latent 0"),
        "latent negative probability": (dict(lprobs=[0.3, -0.3, 0.3]), b"latent 0"),
        "latent negative variance": (dict(lkind=[0, 1], lp1=[0.0, -3.0]), b"negative variance"),
    }
    for name, (change, text) in refusals.items():
        assert _raw(ctx, **{**GOOD, **change}) == -1, name
        err = ctx.lib.twosd_last_error()
        assert b"set_distributions_lintr" in err and text in err, (name, err)
    # k + Q >= 2^31: refused from the shapes alone
    assert _raw(ctx, **{**GOOD, "loff": [0, 2 ** 31 - 6]}) == -5
    # ... and the previous tables are still in use
    np.testing.assert_array_equal(_bits(draw(ctx, N_SMALL, SEED, FIRST, "iid")), _bits(got))
    # the joint and the plain entry points refuse kind 4, leaving the tables in use
    a = [_i32(GOOD["kind"]), _i32(GOOD["nsup"]), _f64(GOOD["vals"]), _f64(GOOD["probs"]), _f64(GOOD["p0"]), _f64(GOOD["p1"])]
    b = [_i32(GOOD["moff"]), _i32(GOOD["mem"]), _i32(GOOD["nreal"]), _f64(GOOD["bp"]), _f64(GOOD["bv"])]
    assert ctx.lib.twosd_set_distributions_joint(ctx.h, 6, *[ptr(v) for v in a], 1, *[ptr(v) for v in b]) == -1
    assert b"unknown kind 4" in ctx.lib.twosd_last_error()
    np.testing.assert_array_equal(_bits(draw(ctx, N_SMALL, SEED, FIRST, ("lhs", 16))),
                                  _bits(_stored(ctx, R.draw(("lhs", 16), dists, blocks, lintr, N_SMALL, SEED, FIRST))))
    # zero LINTR blocks (or NULL) is the joint call: it drops the LINTR tables
    plain_kind = [2, 2, 3, 2, 3, 2]
    assert _raw(ctx, **{**GOOD, "kind": plain_kind, "p1": [1.0, 12.0, 0, 1.0, 0, 1.0]}, nlintr=0) == 0
    ctxb, _ = small("exact", lintr=False)
    want = draw(ctxb, N_SMALL, SEED, FIRST, "antithetic")
    np.testing.assert_array_equal(_bits(draw(ctx, N_SMALL, SEED, FIRST, "antithetic")), _bits(want))
    # twosd_set_distributions drops them too
    assert _raw(ctx, **GOOD) == 0
    sto = small_sto("exact", lintr=False)
    sto.blocks = []
    _, pos = _template()
    sto.indep[pos[4]] = sto.indep[pos[2]] = ("UNIFORM", 0.0, 1.0)
    ctx.set_distributions(sto)
    ctxb.set_distributions(sto)
    np.testing.assert_array_equal(_bits(draw(ctx, N_SMALL, SEED, FIRST, "iid")), _bits(draw(ctxb, N_SMALL, SEED, FIRST, "iid")))
    ctx.close()
    ctxb.close()


# ---- mvnormal_lintr ---------------------------------------------------------------------------------------
def test_mvnormal_lintr_sample_covariance():
    from sqlp_amd import smps, twosd
    S, pos = _template()
    sd = np.array([2.0, 0.5, 3.0])
    corr = np.array([[1.0, 0.8, -0.3], [0.8, 1.0, 0.1], [-0.3, 0.1, 1.0]])
    cov = corr * np.outer(sd, sd)
    mean = np.array([1.0, -2.0, 0.5])
    sto = smps.spStoType("synthetic", {pos[e]: ("UNIFORM", 0.0, 1.0) for e in (0, 2, 4)})
    sto.lintr = [smps.mvnormal_lintr("MVN", "P2", [pos[3], pos[1], pos[5]], mean, cov)]
    ctx = twosd.SDContext(S.sp2, sto, positions=pos)
    ctx.set_distributions(sto)
    got = draw(ctx, MVN_N, MVN_SEED, 0, "iid")[:, [3, 1, 5]]
    se = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / MVN_N)
    z = (np.cov(got.T, bias=True) - cov) / se
    print(f"sample covariance z =\n{np.round(z, 2)}\nmean z = {np.round((got.mean(axis=0) - mean) / (sd / np.sqrt(MVN_N)), 2)}")
    assert np.abs(z).max() <= 6.0
    assert (np.abs(got.mean(axis=0) - mean) <= 6.0 * sd / np.sqrt(MVN_N)).all()
    ctx.close()


# ---- downstream on lands3t at x_EV --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lands3t():
    from sqlp_amd import smps, twosd
    L = R.lands3t()
    ctx = twosd.SDContext(L["sp2"], L["sto"])
    ctx.set_distributions(L["sto"])
    assert ctx.positions == L["positions"]
    ctx.compute_basis(L["x"], smps.mean_values(L["sto"]))
    return L, ctx


@pytest.mark.parametrize("plan", R.LANDS3T_PLANS, ids=plan_name)
def test_evaluate_moments_on_lands3t(plan):
    from sqlp_amd import twosd
    L, ctx = _lands3t()
    x, c1 = L["x"], L["c1"]
    m = twosd.evaluate_moments(ctx, c1, x, R.LANDS3T_SEED, 0, R.LANDS3T_N, sampling=_sampling(plan))
    ref = L["streams"][plan]
    cx = float(np.dot(c1, x))
    assert m.n_bad == 0 and m.n_scenarios == R.LANDS3T_N and m.group == R.group_of(plan)
    z = (m.mean - cx - L["exact"]) / m.std_error
    print(f"{plan_name(plan)}: mean {m.mean:.6f} (restated {cx + ref['mean']:.6f}), standard error {m.std_error:.4f} "
          f"(restated {ref['se']:.4f}), z = {z:.2f}")
    assert abs(m.mean - (cx + ref["mean"])) <= 1e-9 * abs(cx + ref["mean"])
    assert abs(m.std_error - ref["se"]) <= 1e-6 * ref["se"]
    assert abs(z) <= 4.0


def test_evaluate_ci_converges_on_lands3t():
    from sqlp_amd import twosd
    L, ctx = _lands3t()
    r = twosd.evaluate_ci(ctx, L["c1"], L["x"], R.LANDS3T_SEED, batch=1024, n_max=32768, rel_tol=2e-3, z=1.96,
                          sampling=twosd.Sampling.antithetic())
    print(f"evaluate_ci (antithetic): {r.n_scenarios} scenarios, mean {r.mean:.4f}, half-width {r.half_width:.4f}")
    assert r.converged and r.n_bad == 0 and r.half_width <= 2e-3 * abs(r.mean)
    assert abs(r.mean - float(np.dot(L["c1"], L["x"])) - L["exact"]) <= 2.0 * r.half_width + 4 * L["streams"]["antithetic"]["se"]


def test_sampled_cut_equals_the_cpu_cut_on_the_restated_values():
    from oracle import cpu
    from sqlp_amd import twosd
    from tests import instances as I
    L, ctx = _lands3t()
    x, N = L["x"], 512
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, N, R.LANDS3T_SEED, sampling=twosd.Sampling.lhs(16))
    vals = L["streams"][("lhs", 16)]["values"][:N]
    np.testing.assert_array_equal(twosd.get_scenarios(epi), _stored(ctx, vals))
    V = twosd.sdDualVertexSet(ctx)
    obj, st, _ = twosd.solve_push(epi, x, 0, N)
    assert (st == 0).all()
    np.testing.assert_allclose(obj, L["streams"][("lhs", 16)]["obj"][:N], rtol=1e-9)
    cut, mv, ma = twosd._build_cut(epi, x, 0.0, want_argmax=True)
    sp = I.load("lands")["osp2"]
    a, b, omv, oma = cpu.build_cut(sp.r, sp.T, x, V.matrix(), ctx.rows, twosd.get_scenarios(epi) - sp.r[ctx.rows], np.ones(N),
                                   tie_rel=0.0, nthreads=4)
    assert (ma == oma).all(), int((ma != oma).sum())
    assert cut.alpha == pytest.approx(a, rel=1e-8, abs=1e-8)
    np.testing.assert_allclose(cut.beta, b, rtol=1e-8, atol=1e-8 * (1 + np.abs(b).max()))


def test_bootstrap_gap_test_runs_on_antithetic_lintr_pairs():
    from sqlp_amd import master, smps, twosd
    L = R.lands3t()
    sp1 = smps.get_smps_stage_template(L["cor"], L["tim"], 1)
    ctx = twosd.SDContext(L["sp2"], L["sto"])
    ctx.compute_basis(L["x"], smps.mean_values(L["sto"]))
    cell = master.sdCell(sp1, ctx)
    cell.bind_epigraph(twosd.sdEpigraph(ctx, 1.0, 0.0))
    cell.x_candidate = L["x"].copy()
    cell.x_incumbent = L["x"].copy()
    vals = L["streams"]["antithetic"]["values"]
    anti = twosd.Sampling.antithetic()
    it, last = master.sd_run(cell, lambda i: [vals[2 * i:2 * i + 2]], 10, check_every=10, sampling=anti,
                             stop_args=dict(M=8, seed=8), quad_scalar_schedule=master.ConstantQuadScalarSchedule(0.1))
    assert it == 10 and last is not None and last.U.shape == last.L.shape == (9,)
    assert cell.epi[0].num_scenarios == 20
    assert last.gaps[0] >= -1e-8 * (1 + abs(last.U[0])), last.gaps[0]
    print(f"lands3t, antithetic pairs: gap {float(last.gaps[0]):.6f}, fraction {last.fraction}")
    ctx.close()
