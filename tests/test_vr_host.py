"""Variance-reduced streams without a GPU: the ABI's new symbols and plan checks, the whole-group
shard split of sqlp_amd.dist, and self-checks of the numpy reference tests/vr_ref.py (its Philox
against the oracle's C restatement, its i.i.d. stream against the oracle's sampler, the LHS
permutations' bijectivity and uniformity)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import vr_ref as R

NEW_SYMBOLS = ["twosd_add_sampled_scenarios_vr", "twosd_moments_of_values_grouped", "twosd_evaluate_moments_vr",
               "twosd_evaluate_paired_vr", "twosd_evaluate_ci_vr"]


def test_new_symbols_and_struct_layout():
    from sqlp_amd import _lib
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert C.sizeof(_lib.SamplingPlan) == 8
    assert (_lib.SAMPLING_IID, _lib.SAMPLING_ANTITHETIC, _lib.SAMPLING_LHS) == (0, 1, 2)


@pytest.mark.parametrize("mode,group,word", [(7, 1, "mode 7"), (0, 2, "not 2"), (1, 3, "not 3"), (2, 1, "not 1"),
                                             (2, 257, "not 257"), (2, -4, "not -4")])
def test_plan_is_checked_before_anything_else(mode, group, word):
    """The plan check needs no context: both fields of the struct reach the library where the
    header puts them, and the offending value is in the error text."""
    from sqlp_amd import _lib
    lib = _lib.load()
    plan = _lib.SamplingPlan(mode, group)
    out = _lib.Moments()
    assert lib.twosd_add_sampled_scenarios_vr(None, 0, 4, 1, 0, None, C.byref(plan)) == -1
    assert word in lib.twosd_last_error().decode()
    assert lib.twosd_evaluate_moments_vr(None, None, 0, 512, 1, C.byref(out), C.byref(plan)) == -1
    assert word in lib.twosd_last_error().decode()


def test_misaligned_ranges_are_arg_errors_without_a_context():
    from sqlp_amd import _lib
    lib = _lib.load()
    out, hw, conv = _lib.Moments(), C.c_double(), C.c_int()
    anti, lhs3 = _lib.SamplingPlan(1, 2), _lib.SamplingPlan(2, 3)
    assert lib.twosd_add_sampled_scenarios_vr(None, 0, 4, 1, 7, None, C.byref(anti)) == -1
    assert "first_index = 7" in lib.twosd_last_error().decode()
    assert lib.twosd_add_sampled_scenarios_vr(None, 0, 5, 1, 6, None, C.byref(lhs3)) == -1
    assert "N = 5" in lib.twosd_last_error().decode()
    assert lib.twosd_evaluate_moments_vr(None, None, 3, 10, 1, C.byref(out), C.byref(lhs3)) == -1
    assert "count = 10" in lib.twosd_last_error().decode()
    assert lib.twosd_evaluate_ci_vr(None, None, 1, 0, 3, 300, 1.96, 0.1, 0.0, 0.0, C.byref(out), C.byref(hw), C.byref(conv),
                                    C.byref(lhs3)) == -1
    assert "batch = 3" in lib.twosd_last_error().decode()                 # one group only
    assert lib.twosd_evaluate_ci_vr(None, None, 1, 0, 7, 300, 1.96, 0.1, 0.0, 0.0, C.byref(out), C.byref(hw), C.byref(conv),
                                    C.byref(anti)) == -1
    assert "batch = 7" in lib.twosd_last_error().decode()
    assert lib.twosd_moments_of_values_grouped(None, 10, 3, None, None, C.byref(out)) == -1
    assert "n = 10" in lib.twosd_last_error().decode()
    assert lib.twosd_moments_of_values_grouped(None, 10, 257, None, None, C.byref(out)) == -1


def test_sampling_value():
    from sqlp_amd import twosd
    assert twosd.Sampling.iid().group == 1 and twosd.Sampling.antithetic().group == 2 and twosd.Sampling.lhs(64).group == 64
    assert (twosd.Sampling.lhs(3).mode, twosd.Sampling.antithetic().mode, twosd.Sampling().mode) == (2, 1, 0)
    m = twosd.Moments(5, 1, 2.0, 1.0, 0.0, 3.0, 64)
    assert m.n_scenarios == 320 and twosd.Moments(5).n_scenarios == 5
    assert m.merge(twosd.Moments(group=64)) == m
    with pytest.raises(ValueError):
        m.merge(twosd.Moments(3, 0, 1.0, 0.5, 0.0, 2.0))
    r = twosd.EvaluateCI(1.0, 0.1, 10, 0, True, m, 64)
    assert r.n_scenarios == 640


# ---- the whole-group shard split ---------------------------------------------------------------
@pytest.mark.parametrize("lo,ngroups,world,G", [(0, 8, 2, 2), (12, 7, 8, 3), (0, 1000, 8, 3), (64, 3, 8, 64), (0, 5, 1, 256),
                                                (6, 0, 4, 3), (0, 4096, 3, 1)])
def test_group_shard_ranges(lo, ngroups, world, G):
    from sqlp_amd.dist import group_shard_ranges, shard_range
    hi = lo + ngroups * G
    rs = group_shard_ranges(lo, hi, world, G)
    assert len(rs) == world and rs[0][0] == lo and rs[-1][1] == hi
    for (a, b), (c, _) in zip(rs, rs[1:] + [(hi, hi)]):
        assert a <= b == c                                         # contiguous in rank order: disjoint, covering
        assert (a - lo) % G == 0 and (b - lo) % G == 0             # whole groups
    sizes = [(b - a) // G for a, b in rs]
    assert sum(sizes) == ngroups and max(sizes) - min(sizes) <= 1
    if ngroups < world:
        assert sizes.count(0) == world - ngroups                   # fewer groups than ranks: empty ranges
    if G == 1:
        assert rs == [tuple(lo + v for v in shard_range(ngroups, r, world)) for r in range(world)]


def test_group_shard_ranges_rejects_partial_groups():
    from sqlp_amd.dist import group_shard_ranges
    with pytest.raises(ValueError):
        group_shard_ranges(0, 10, 2, 3)
    with pytest.raises(ValueError):
        group_shard_ranges(1, 7, 2, 3)


# ---- the reference's own checks ----------------------------------------------------------------
def test_ref_philox_matches_the_oracle():
    from oracle import cpu
    rng = np.random.default_rng(3)
    for _ in range(20):
        ctr = rng.integers(0, 2 ** 32, size=4, dtype=np.uint64)
        seed = int(rng.integers(0, 2 ** 63, dtype=np.uint64))
        want = cpu.philox4x32_10(ctr.astype(np.uint32), np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32))
        got = R.philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], seed)
        assert [int(np.asarray(w).ravel()[0]) for w in got] == [int(w) for w in want]


def _mixed():
    from tests import synth_cases as SC
    from tests.test_gpu_sampler import _mixed_sto
    S = SC.template("e")
    sto = _mixed_sto(S)
    from sqlp_amd.smps import spSmpsPosition
    pos = [spSmpsPosition(c, r) for c, r in S.positions]
    return S, sto, pos


def test_ref_iid_stream_matches_the_oracle_sampler():
    """The restated i.i.d. stream against oracle/sampler.c: what ANTITHETIC's even rows and the u1
    of LHS build on.  A first index that carries into the high counter word."""
    from oracle import cpu
    S, sto, pos = _mixed()
    N, seed, first = 600, 0x9E3779B97F4A7C15, 2 ** 32 - 300
    tv = np.asarray(S.r[S.rows], dtype=np.float64)
    want = cpu.sample_deltas(sto, pos, tv, N, seed, first) + tv
    got = R.iid(R.dists_of(sto, pos), N, seed, first)
    kinds = np.array([sto.indep[p][0] for p in pos])
    np.testing.assert_array_equal(got[:, kinds != "NORMAL"], want[:, kinds != "NORMAL"])
    np.testing.assert_allclose(got[:, kinds == "NORMAL"], want[:, kinds == "NORMAL"], rtol=1e-12, atol=1e-12)


def test_ref_antithetic_mirrors():
    S, sto, pos = _mixed()
    d = R.dists_of(sto, pos)
    a = R.antithetic(d, 512, 11, 10)
    i = R.iid(d, 512, 11, 10)
    np.testing.assert_array_equal(a[0::2], i[0::2])
    for e, dist in enumerate(d):
        if dist[0] == "UNIFORM":
            assert np.abs(a[0::2, e] + a[1::2, e] - (dist[1] + dist[2])).max() <= 2 * np.spacing(abs(dist[1]) + abs(dist[2]))
        if dist[0] == "NORMAL":
            np.testing.assert_allclose(a[0::2, e] + a[1::2, e], 2 * dist[1], rtol=1e-14)


@pytest.mark.parametrize("S", [2, 3, 64, 256])
def test_ref_lhs_permutations_are_bijections(S):
    perm = R.lhs_permutations(S, (2 ** 32 - 2) + np.arange(5), 8, 0xC0FFEE1234567)
    assert perm.shape == (5, 8, S)
    assert (np.sort(perm, axis=2) == np.arange(S)).all()
    u = R.lhs_uniforms(S, 4 * S, 8, 99, first=8 * S)
    strata = np.floor(u * S).astype(int).reshape(4, S, 8)
    assert (np.sort(strata, axis=1) == np.arange(S)[None, :, None]).all() and u.max() < 1.0 and u.min() >= 0.0


def test_ref_lhs_permutations_are_uniform():
    """S = 4 over 4096 blocks: chi^2 of the 24 permutation frequencies below the 99.99 % quantile
    of chi^2 with 23 degrees of freedom (57.0)."""
    perm = R.lhs_permutations(4, np.arange(4096), 1, 20260101)[:, 0, :]
    index = {p: i for i, p in enumerate(itertools.permutations(range(4)))}
    counts = np.bincount([index[tuple(int(v) for v in row)] for row in perm], minlength=24)
    expect = 4096 / 24
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print(f"chi^2 = {chi2:.2f}")
    assert chi2 < 57.0


def test_ref_ncdfinv():
    """Lower tail: Phi(z) returns u to a few ulp (erfc is relatively accurate there); upper tail
    by symmetry; the stdlib's AS241 agrees to its own 1e-9."""
    import math
    from statistics import NormalDist
    for u in [2.0 ** -54, 1e-12, 0.01, 0.3, 0.4999999, 0.5]:
        z = R.ncdfinv(u)
        # one ulp of z moves Phi by about z^2 ulp in the tail (d log Phi / d log z ~ z^2)
        assert abs(0.5 * math.erfc(-z / math.sqrt(2.0)) - u) <= 4 * (1 + z * z) * np.spacing(u)
        assert abs(z - NormalDist().inv_cdf(u)) <= 1e-9 * max(1.0, abs(z))
    assert R.ncdfinv(0.5) == 0.0 and R.ncdfinv(0.25) == -R.ncdfinv(0.75)
    assert R.ncdfinv(R.ONE_MINUS) == -R.ncdfinv(2.0 ** -53) and 8.0 < R.ncdfinv(R.ONE_MINUS) < 8.3


def test_ref_group_means_order_and_mask():
    v = 1e9 + np.random.default_rng(0).normal(size=12)
    m = R.group_means(v, 3)
    for b in range(4):
        K, s = v[3 * b], 0.0
        for i in range(3):
            s = s + (v[3 * b + i] - K)
        assert m[b] == K + s / 3.0
    st = np.zeros(12, dtype=np.int32)
    st[4] = 2
    w = v.copy()
    w[3:6] = np.nan
    means, bad = R.grouped(w, st, 3)
    assert bad == 1 and np.isfinite(means).all() and (means == m[[0, 2, 3]]).all()
