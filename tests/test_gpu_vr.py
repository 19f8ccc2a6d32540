"""Variance-reduced scenario streams on the device: the antithetic and Latin
hypercube sampler kernels against the numpy restatement tests/vr_ref.py (DISCRETE / UNIFORM bit for
bit, NORMAL within the project's 1e-12), the grouped-means kernel through moments_of_values(group=G),
and the estimators under a sampling plan on lands at x_EV.

Tolerances: the sampler's and the moments kernel's are those of tests/test_gpu_sampler.py and
tests/test_gpu_evaluate_ci.py (1e-12 on NORMAL values, on the mean and on well-conditioned m2; 1e-9
on m2 of ill-conditioned data; against a host chain of LP objectives 1e-9 (1 + |mean|) and 1e-6 on
the variance).  The group means themselves are compared bit for bit: vr_ref.group_means restates
their order of operations."""
import functools
import os
import struct

import numpy as np
import pytest

from tests import instances as I
from tests import vr_ref as R

pytestmark = pytest.mark.gpu

SEED = 777


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


def _ld(v):
    v = np.asarray(v, dtype=np.longdouble)
    mean = v.sum() / v.size
    return int(v.size), float(mean), float(((v - mean) ** 2).sum()), float(v.min()), float(v.max())


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def _bytes(m):
    return struct.pack("<qqdddd", m.n, m.n_bad, m.mean, m.m2, m.min, m.max)


def _arg_error(fn):
    from sqlp_amd._lib import TwoSDError
    with pytest.raises(TwoSDError) as ei:
        fn()
    assert ei.value.code == -1
    return str(ei.value)


# ---- the mixed template: the three kinds over k = 8 rhs rows ---------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed(S_equal=0):
    """Context on generated template "e" with _mixed_sto's distributions; S_equal > 0 replaces the
    last element by a DISCRETE one with S_equal equally likely support points."""
    from sqlp_amd import twosd
    from tests import synth_cases as SC
    from tests.test_gpu_sampler import _mixed_sto
    S = SC.template("e")
    sto = _mixed_sto(S)
    if S_equal:
        last = list(sto.indep.keys())[-1]
        sto.indep[last] = ("DISCRETE", [float(v) for v in range(S_equal)], [1.0 / S_equal] * S_equal)
    ctx = twosd.SDContext(S.sp2, sto)
    ctx.set_distributions(sto)
    dists = R.dists_of(sto, ctx.positions)
    kinds = np.array([d[0] for d in dists])
    assert set(kinds) == {"DISCRETE", "NORMAL", "UNIFORM"} and ctx.k == 8
    return ctx, dists, kinds


def _draw(ctx, N, seed, first, sampling):
    from sqlp_amd import twosd
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, N, seed, first_index=first, sampling=sampling)
    assert epi.num_scenarios == N
    return twosd.get_scenarios(epi)


def _match_ref(ctx, got, ref, dists, kinds):
    """DISCRETE / UNIFORM bit for bit; NORMAL compared in z within 1e-12 max(1, |z|).  An epigraph
    stores value - template and get_scenarios adds the template back: the reference values take
    the same two roundings (as the oracle's sample_deltas + template does for the i.i.d. stream)."""
    ref = (ref - ctx.template_values) + ctx.template_values
    exact = kinds != "NORMAL"
    np.testing.assert_array_equal(got[:, exact], ref[:, exact])
    for e in np.nonzero(~exact)[0]:
        mean, sd = dists[e][1], np.sqrt(dists[e][2])
        zg, zr = (got[:, e] - mean) / sd, (ref[:, e] - mean) / sd
        err = np.abs(zg - zr) / np.maximum(1.0, np.abs(zr))
        print(f"NORMAL element {e}: max z error {err.max():.3e} (|z| up to {np.abs(zr).max():.2f})")
        assert err.max() <= 1e-12


# ---- 1. IID and NULL plans are the i.i.d. sampler ---------------------------------------------------
def test_iid_plan_is_the_iid_stream():
    from sqlp_amd import twosd
    ctx, _, _ = _mixed()
    N, seed = 1000, 0x9E3779B97F4A7C15
    want = _draw(ctx, N, seed, 7, None)
    np.testing.assert_array_equal(_draw(ctx, N, seed, 7, twosd.Sampling.iid()), want)
    np.testing.assert_array_equal(_draw(ctx, N, seed, 7, twosd.Sampling()), want)
    # a NULL plan through the new entry point itself
    import ctypes as C
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    assert ctx.lib.twosd_add_sampled_scenarios_vr(ctx.h, epi.index, N, C.c_uint64(seed), C.c_uint64(7), None, None) == 0
    np.testing.assert_array_equal(twosd.get_scenarios(epi), want)


# ---- 2. antithetic pairs ---------------------------------------------------------------------------
def test_antithetic_stream():
    from sqlp_amd import twosd
    ctx, dists, kinds = _mixed()
    N, seed, first = 2048, 0x9E3779B97F4A7C15, 10
    anti = twosd.Sampling.antithetic()
    got = _draw(ctx, N, seed, first, anti)
    iid = _draw(ctx, N, seed, first, None)
    np.testing.assert_array_equal(got[0::2], iid[0::2])                 # even members: the i.i.d. draws
    _match_ref(ctx, got, R.antithetic(dists, N, seed, first), dists, kinds)
    for e in np.nonzero(kinds == "UNIFORM")[0]:
        left, right = dists[e][1], dists[e][2]
        assert np.abs(got[0::2, e] + got[1::2, e] - (left + right)).max() <= 2 * np.spacing(abs(left) + abs(right))
    assert (got[1::2] != iid[1::2]).any(axis=0).sum() >= 7              # all but the one-point support differ
    two = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(two, 600, seed, first_index=first, sampling=anti)
    twosd.add_sampled_scenarios(two, N - 600, seed, first_index=first + 600, sampling=anti)
    np.testing.assert_array_equal(twosd.get_scenarios(two), got)
    assert "first_index = 11" in _arg_error(lambda: _draw(ctx, 4, seed, 11, anti))
    assert "N = 5" in _arg_error(lambda: _draw(ctx, 5, seed, 10, anti))
    assert "not 3" in _arg_error(lambda: _draw(ctx, 6, seed, 0, twosd.Sampling(1, 3)))


# ---- 3. Latin hypercube blocks ---------------------------------------------------------------------
@pytest.mark.parametrize("S,blocks", [(2, 4), (3, 4), (64, 4), (256, 4), (64, 64)])
def test_lhs_stream(S, blocks):
    """The first index sits two blocks below 2^32, so the scenario counter carries into its high
    word inside the batch; 64 blocks x 8 elements fill more than one thread block of the kernel."""
    from sqlp_amd import twosd
    ctx, dists, kinds = _mixed(S)
    N, seed, first = S * blocks, 0xC0FFEE123456789, (2 ** 32 // S - 2) * S
    plan = twosd.Sampling.lhs(S)
    got = _draw(ctx, N, seed, first, plan)
    _match_ref(ctx, got, R.lhs(dists, S, N, seed, first), dists, kinds)
    per_block = got.reshape(blocks, S, ctx.k)
    for e in np.nonzero(kinds == "UNIFORM")[0]:
        left, right = dists[e][1], dists[e][2]
        strata = np.floor((per_block[:, :, e] - left) / (right - left) * S).astype(int)
        assert (np.sort(strata, axis=1) == np.arange(S)).all()          # one draw per stratum, every block
    assert (np.sort(per_block[:, :, ctx.k - 1], axis=1) == np.arange(S, dtype=float)).all()   # S equally likely points: each once
    cut = (blocks // 2) * S
    two = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(two, cut, seed, first_index=first, sampling=plan)
    twosd.add_sampled_scenarios(two, N - cut, seed, first_index=first + cut, sampling=plan)
    np.testing.assert_array_equal(twosd.get_scenarios(two), got)
    assert f"first_index = {first + 1}" in _arg_error(lambda: _draw(ctx, S, seed, first + 1, plan))
    assert f"N = {S + 1}" in _arg_error(lambda: _draw(ctx, S + 1, seed, first, plan))


def test_lhs_group_bounds():
    from sqlp_amd import twosd
    ctx, _, _ = _mixed()
    assert "not 1" in _arg_error(lambda: _draw(ctx, 4, 1, 0, twosd.Sampling.lhs(1)))
    assert "not 257" in _arg_error(lambda: _draw(ctx, 257, 1, 0, twosd.Sampling.lhs(257)))
    assert "mode 9" in _arg_error(lambda: _draw(ctx, 4, 1, 0, twosd.Sampling(9, 2)))


# ---- 4. the grouped-means kernel through moments_of_values(group=G) ---------------------------------
@pytest.mark.parametrize("ngroups", [1, 255, 257, 1000])
@pytest.mark.parametrize("G", [2, 3, 64, 256])
def test_grouped_moments_kernel(G, ngroups):
    """1e9 + N(0, 1): the group sums cancel nine digits.  255 / 257 / 1000 groups straddle the 256
    blocks of the moments kernel (and 257 / 1000 the 256-thread blocks of the means kernel)."""
    from sqlp_amd import twosd
    ctx, _, _ = _mixed()
    n = G * ngroups
    v = 1e9 + np.random.default_rng(1000 * G + ngroups).normal(size=n)
    m = twosd.moments_of_values(ctx, v, group=G)
    means, bad = R.grouped(v, None, G)
    cnt, mean, m2, mn, mx = _ld(means)
    print(f"G {G} x {ngroups}: mean rel err {_rel(m.mean, mean):.2e}, m2 rel err {_rel(m.m2, m2) if m2 else 0.0:.2e}")
    assert (m.n, m.n_bad, m.min, m.max, m.group, m.n_scenarios) == (ngroups, 0, mn, mx, G, n)   # min / max: the means' own bits
    assert abs(m.mean - mean) <= 1e-12 * abs(mean)
    if ngroups == 1:
        assert m.m2 == 0.0 and m.mean == means[0]
    else:
        assert abs(m.m2 - m2) <= 1e-9 * m2
    assert _bytes(twosd.moments_of_values(ctx, v, group=G)) == _bytes(m)       # the same bits on every run
    assert _bytes(twosd.moments_of_values(ctx, v, np.zeros(n, dtype=np.int32), group=G)) == _bytes(m)
    # well-conditioned data: the moments step itself to 1e-12
    w = 250.0 + 40.0 * np.random.default_rng(G + ngroups).normal(size=n)
    mw = twosd.moments_of_values(ctx, w, group=G)
    _, mean, m2, _, _ = _ld(R.group_means(w, G))
    assert abs(mw.mean - mean) <= 1e-12 * abs(mean) and (ngroups == 1 or abs(mw.m2 - m2) <= 1e-12 * m2)
    # one non-optimal entry removes exactly its group; that group's NaNs never reach a sum
    st = np.zeros(n, dtype=np.int32)
    gb = ngroups // 2
    st[gb * G + G - 1] = 2
    vb = v.copy()
    vb[gb * G: (gb + 1) * G] = np.nan
    mb = twosd.moments_of_values(ctx, vb, st, group=G)
    means_b, bad = R.grouped(vb, st, G)
    assert bad == 1 and (mb.n, mb.n_bad) == (ngroups - 1, 1)
    if ngroups == 1:
        assert (mb.mean, mb.m2, mb.min, mb.max) == (0.0, 0.0, np.inf, -np.inf)
    else:
        cnt, mean, m2, mn, mx = _ld(means_b)
        assert np.isfinite([mb.mean, mb.m2]).all() and (mb.min, mb.max) == (mn, mx)
        assert abs(mb.mean - mean) <= 1e-12 * abs(mean) and (cnt == 1 or abs(mb.m2 - m2) <= 1e-9 * m2)
    assert f"n = {n + 1}" in _arg_error(lambda: twosd.moments_of_values(ctx, np.zeros(n + 1), group=G))


def test_grouped_moments_group_of_one_is_the_ungrouped_call():
    import ctypes as C
    from sqlp_amd import _lib, twosd
    ctx, _, _ = _mixed()
    v = 1e9 + np.random.default_rng(5).normal(size=777)
    out = _lib.Moments()
    assert ctx.lib.twosd_moments_of_values_grouped(ctx.h, C.c_int64(v.size), 1, v.ctypes.data_as(C.c_void_p), None, C.byref(out)) == 0
    assert _bytes(out) == _bytes(twosd.moments_of_values(ctx, v))


# ---- 5 - 7. the estimators on lands at x_EV --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lands():
    from sqlp_amd import smps, twosd
    inst = I.load("lands")
    ctx = twosd.SDContext(inst["sp2"], inst["sto"])
    x = I.x_ev("lands")
    ctx.compute_basis(x, smps.mean_values(inst["sto"]))
    ctx.set_distributions(inst["sto"])
    return ctx, x


def _plans():
    from sqlp_amd import twosd
    return {"antithetic": twosd.Sampling.antithetic(), "lhs64": twosd.Sampling.lhs(64)}


@pytest.mark.parametrize("which", ["antithetic", "lhs64"])
def test_evaluate_moments_under_a_plan(which):
    """evaluate_moments(sampling=) == the chain: the plan's scenarios into an epigraph, solve_batch,
    grouped moments of those objectives on the host."""
    from sqlp_amd import twosd
    ctx, x = _lands()
    plan = _plans()[which]
    G, N = plan.group, 4096
    zero = np.zeros(len(x))
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, N, SEED, sampling=plan)
    obj, _, _, st = twosd.solve_batch(epi, x, want_pi=False)
    assert (st == 0).all()
    means, bad = R.grouped(obj, st, G)
    n, mean, m2, mn, mx = _ld(means)
    m = twosd.evaluate_moments(ctx, zero, x, SEED, 0, N, sampling=plan)
    print(f"{which}: n {m.n} groups, mean {m.mean!r} (chain {mean!r}), variance rel {_rel(m.variance, m2 / (n - 1)):.2e}")
    assert (m.n, m.n_bad, m.group, m.n_scenarios) == (N // G, 0, G, N)
    assert abs(m.mean - mean) <= 1e-9 * (1 + abs(mean))
    assert _rel(m.variance, m2 / (n - 1)) <= 1e-6
    assert abs(m.min - mn) <= 1e-9 * (1 + abs(mn)) and abs(m.max - mx) <= 1e-9 * (1 + abs(mx))
    assert twosd.evaluate_moments(ctx, zero, x, SEED, 0, N, sampling=plan) == m      # the same bits on every run
    with _env("TWOSD_EVAL_CHUNK", "1000"):                       # 1000 -> 960 (lhs64) / 1000 (pairs): whole groups
        mc = twosd.evaluate_moments(ctx, zero, x, SEED, 0, N, sampling=plan)
    assert (mc.n, mc.n_bad) == (m.n, 0) and abs(mc.mean - m.mean) <= 1e-9 * (1 + abs(m.mean))
    assert _rel(mc.m2, m.m2) <= 1e-6 and (mc.min, mc.max) == (m.min, m.max)
    # shards on group boundaries merge to the whole; c'x enters mean / min / max only
    a = 15 * 64
    parts = twosd.evaluate_moments(ctx, zero, x, SEED, 0, a, sampling=plan).merge(
        twosd.evaluate_moments(ctx, zero, x, SEED, a, N - a, sampling=plan))
    assert (parts.n, parts.group) == (m.n, G) and abs(parts.mean - m.mean) <= 1e-12 * (1 + abs(m.mean))
    c1 = np.linspace(1.0, 2.0, len(x))
    cx = float(c1 @ x)
    mcx = twosd.evaluate_moments(ctx, c1, x, SEED, 0, N, sampling=plan)
    assert (mcx.mean, mcx.min, mcx.max, mcx.m2) == (m.mean + cx, m.min + cx, m.max + cx, m.m2)
    assert "first = 1" in _arg_error(lambda: twosd.evaluate_moments(ctx, zero, x, SEED, 1, N, sampling=plan))
    assert "count = " in _arg_error(lambda: twosd.evaluate_moments(ctx, zero, x, SEED, 0, N + 1, sampling=plan))
    # paired at xa = xb: a zero difference record over the same groups
    pa, pb, d = twosd.evaluate_paired(ctx, zero, x, x, SEED, 0, N, sampling=plan)
    assert pa == m and pb == m
    assert (d.n, d.n_bad, d.mean, d.m2, d.min, d.max, d.group) == (m.n, 0, 0.0, 0.0, 0.0, 0.0, G)


def test_variance_reduction_is_real():
    """lands at x_EV, 16384 scenarios of stream 777 (the reference streams solved by the C oracle on
    the host give i.i.d. : antithetic : LHS-64 standard errors 0.565 : 0.048 : 0.054)."""
    from sqlp_amd import twosd
    ctx, x = _lands()
    zero = np.zeros(len(x))
    N = 16384
    iid = twosd.evaluate_moments(ctx, zero, x, SEED, 0, N)
    res = {k: twosd.evaluate_moments(ctx, zero, x, SEED, 0, N, sampling=p) for k, p in _plans().items()}
    z999 = 3.2905267314919255
    for k, m in res.items():
        print(f"{k}: std_error {m.std_error:.5f} vs i.i.d. {iid.std_error:.5f} (ratio {iid.std_error / m.std_error:.2f}), "
              f"mean {m.mean:.4f} vs {iid.mean:.4f}")
        assert m.n_scenarios == iid.n == N
        assert m.std_error < iid.std_error
        assert abs(m.mean - iid.mean) <= z999 * (m.std_error + iid.std_error)
    a, b = res["antithetic"], res["lhs64"]
    assert abs(a.mean - b.mean) <= z999 * (a.std_error + b.std_error)


@pytest.mark.parametrize("which", ["antithetic", "lhs64"])
def test_evaluate_ci_under_a_plan(which):
    from sqlp_amd import dist as sdist
    from sqlp_amd import twosd
    ctx, x = _lands()
    plan = _plans()[which]
    G = plan.group
    zero = np.zeros(len(x))
    kw = dict(batch=1024, n_max=6144, rel_tol=0.009, z=1.96)
    iid = twosd.evaluate_ci(ctx, zero, x, SEED, **kw)
    r = twosd.evaluate_ci(ctx, zero, x, SEED, sampling=plan, **kw)
    print(f"{which}: stops at {r.n_scenarios} scenarios ({r.n} groups), half-width {r.half_width!r}; i.i.d. at {iid.n}")
    assert iid.converged and r.converged and r.n_bad == 0
    assert r.n_scenarios <= iid.n_scenarios and r.group == G and r.n == r.n_scenarios // G
    hw = 1.96 * float(np.sqrt(r.moments.m2 / (r.n - 1) / r.n))
    assert r.half_width == hw or _rel(r.half_width, hw) <= 1e-15
    assert r.half_width <= 0.009 * abs(r.mean)
    whole = twosd.evaluate_moments(ctx, zero, x, SEED, 0, r.n_scenarios, sampling=plan)
    assert (whole.n, whole.min, whole.max) == (r.n, r.moments.min, r.moments.max)
    assert abs(whole.mean - r.moments.mean) <= 1e-12 * (1 + abs(whole.mean)) and _rel(r.moments.m2, whole.m2) <= 1e-12
    # n_max is clipped down to whole groups; the cap ends the run
    capped = twosd.evaluate_ci(ctx, zero, x, SEED, batch=2 * G, n_max=5 * G + 1, rel_tol=0.0, z=1.96, sampling=plan)
    assert (capped.n, capped.converged) == (5, False)
    assert "batch = " in _arg_error(lambda: twosd.evaluate_ci(ctx, zero, x, SEED, batch=G, n_max=6144, sampling=plan))
    assert "batch = " in _arg_error(lambda: twosd.evaluate_ci(ctx, zero, x, SEED, batch=4 * G + 1, n_max=6144, sampling=plan))
    # one rank of the sharded form takes the same decision on the same moments
    s = sdist.evaluate_ci_sharded(ctx, zero, x, SEED, sampling=plan, **kw)
    assert (s.n, s.n_bad, s.converged, s.group) == (r.n, 0, True, G) and abs(s.mean - r.mean) <= 1e-12 * (1 + abs(r.mean))
