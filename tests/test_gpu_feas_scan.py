"""The violation scan (twosd_feas_scan, feas_scan_kernel) against the restated score of the C oracle,
bit for bit: oracle.cpu.build_cut called with the one-row vertex set V = F[j:j+1] returns the scores
of ray j in max_val.  F is filled by hand with normalised random vectors of a ray's sign pattern on
the generated incomplete-recourse template (tests/feas_cases.py; random T elements in every case).

Shapes: J in {1, 3, 64, 65} (one ray, a partial tile, a full tile, a second tile), N in {1, 63, 64, 65,
1000} (around the 64-scenario tile; several blocks), k in {1, 3, 70} (70: two 64-element slices)."""
import functools
import os

import numpy as np
import pytest

from tests import feas_cases as FC

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# k: (m_lp, k, boxed, seed, amplitude) of the template
K_CASES = {1: (20, 1, False, 31, 1.0), 3: (65, 3, True, 32, 4.0), 70: (130, 70, True, 33, 2.0)}
JS, NS = [1, 3, 64, 65], [1, 63, 64, 65, 1000]


@functools.lru_cache(maxsize=None)
def _setup(k):
    from sqlp_amd import twosd
    S = FC.incomplete_template(*K_CASES[k], cid=f"scan{k}")
    assert (S.cols >= 0).any()                                            # T elements
    ctx = twosd.SDContext(S.sp2, positions=S.positions)
    assert (ctx.m_lp, ctx.k) == (S.m_lp, k)
    rays = FC.random_rays(S, max(JS), seed=k)
    rays.setflags(write=False)
    K = S.canon
    assert not K.s.any()                                                  # no shift: the canonical r is the template's own
    Tl = np.vstack([S.T, np.zeros((S.nb, FC.N1))])
    return S, ctx, rays, K.r.copy(), Tl


@functools.lru_cache(maxsize=None)
def _reference(k, N):
    """(values with a planted tie, scores J x N of the oracle) at X0, computed once per (k, N)."""
    from oracle import cpu
    S, _, rays, r, Tl = _setup(k)
    vals = FC.values(S, N, seed=7)

    def scores(v):
        DR = FC.deltas(S, FC.X0, v)
        return np.array([cpu.build_cut(r, Tl, FC.X0, rays[j:j + 1], S.rows, DR, np.ones(len(v)), nthreads=1)[2] for j in range(len(rays))])

    if N >= 3:                                                            # an exact tie at ray 0's maximum: two identical scenarios
        s0 = int(np.argmax(scores(vals)[0]))
        vals[N - 1 if s0 != N - 1 else 0] = vals[s0]
    sc = scores(vals)
    vals.setflags(write=False)
    sc.setflags(write=False)
    return vals, sc


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


@pytest.mark.parametrize("k", list(K_CASES))
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("J", JS)
def test_scan_equals_the_oracle_scores(J, N, k):
    from sqlp_amd import twosd
    S, ctx, rays, r, Tl = _setup(k)
    vals, sc = _reference(k, N)
    sc = sc[:J]
    x = FC.X0
    F = twosd.sdFeasRaySet(ctx)
    F.clear()
    np.testing.assert_array_equal(F.push_batch(rays[:J]), np.arange(J))
    np.testing.assert_array_equal(F.get(), rays[:J])
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals)
    got = twosd.feas_scan(epi, x)
    np.testing.assert_array_equal(got.ray_max, sc.max(axis=1))            # bit for bit
    np.testing.assert_array_equal(got.ray_arg, sc.argmax(axis=1))         # the lowest index attaining it
    if N >= 3:
        tie = np.flatnonzero(sc[0] == sc[0].max())
        assert len(tie) >= 2 and got.ray_arg[0] == tie[0]
    np.testing.assert_array_equal(got.cut_off, (sc > 0).any(axis=0))
    assert got.n_cut_off == int((sc > 0).any(axis=0).sum())
    # the row of (j, ray_arg[j]): alpha + beta'x is a re-association of the same terms
    worst = 0.0
    for j in range(J):
        Tw, rw = FC.scenario_T_r(S, vals[got.ray_arg[j]])
        Tw = np.vstack([Tw, np.zeros((S.nb, FC.N1))])
        rw = np.concatenate([rw, S.canon.r[S.m2:]])
        sig = rays[j]
        mag = float(np.abs(sig) @ (np.abs(rw) + np.abs(Tw) @ np.abs(x)))
        np.testing.assert_allclose(got.alpha[j], sig @ rw, rtol=0, atol=4 * EPS * mag)
        np.testing.assert_allclose(got.beta[j], -Tw.T @ sig, rtol=0, atol=4 * EPS * mag)
        err = abs(got.alpha[j] + got.beta[j] @ x - got.ray_max[j])
        worst = max(worst, err / (EPS * mag))
        assert err <= 4 * EPS * mag, (j, err, mag)
    # a sub-range: arg is an index of the epigraph
    if N == 1000 and J == 3:
        sub = twosd.feas_scan(epi, x, first=100, count=130)
        np.testing.assert_array_equal(sub.ray_max, sc[:, 100:230].max(axis=1))
        np.testing.assert_array_equal(sub.ray_arg, 100 + sc[:, 100:230].argmax(axis=1))
        np.testing.assert_array_equal(sub.cut_off, (sc[:, 100:230] > 0).any(axis=0))
    # identical under other grids
    for blocks in ("1", "3"):
        with _env(TWOSD_FEAS_BLOCKS=blocks):
            g2 = twosd.feas_scan(epi, x)
        for a, b in zip((got.ray_max, got.ray_arg, got.alpha, got.beta, got.cut_off), (g2.ray_max, g2.ray_arg, g2.alpha, g2.beta, g2.cut_off)):
            np.testing.assert_array_equal(a, b)
        assert g2.n_cut_off == got.n_cut_off
    print(f"FEAS scan J={J} N={N} k={k}: cut off {got.n_cut_off}/{N}, worst |alpha + beta'x - max| = {worst:.2f} eps * magnitude")


def test_scan_with_an_empty_ray_set_is_a_state_error():
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    S, ctx, rays, _, _ = _setup(3)
    twosd.sdFeasRaySet(ctx).clear()
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, FC.values(S, 4))
    with pytest.raises(TwoSDError) as e:
        twosd.feas_scan(epi, FC.X0)
    assert e.value.code == -3


def test_ray_set_dedup_refusal_and_reset():
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    S, ctx, rays, _, _ = _setup(3)
    F = twosd.sdFeasRaySet(ctx)
    F.clear()
    idx = F.push_batch(np.vstack([rays[:3], 2.5 * rays[1:2], rays[4:5], rays[0:1] * (1 + 2.0 ** -40)]))
    np.testing.assert_array_equal(idx, [0, 1, 2, 1, 3, 0])                # first occurrence kept, scaling ignored
    assert F.size == 4
    bad = rays[:2].copy()
    bad[1] = 0.0
    with pytest.raises(TwoSDError) as e:
        F.push_batch(bad)
    assert e.value.code == -1 and F.size == 4                             # nothing pushed
    bad[1, 0] = np.nan
    with pytest.raises(TwoSDError):
        F.push_batch(bad)
    assert F.size == 4
    # the set goes with the positions and with the template (a context without scenarios: positions can be set again)
    c2 = twosd.SDContext(S.sp2, positions=S.positions)
    F2 = twosd.sdFeasRaySet(c2)
    F2.push_batch(rays[:5])
    assert F2.size == 5
    c2.set_positions(S.positions)
    assert F2.size == 0
    F2.push_batch(rays[:2])
    c2._set_problem(S.sp2, positions=S.positions)
    assert F2.size == 0
    c2.close()


def test_a_full_ray_set_is_unsupported():
    from sqlp_amd import _lib, twosd
    from sqlp_amd._lib import TwoSDError
    S, ctx, _, _, _ = _setup(1)
    F = twosd.sdFeasRaySet(ctx)
    F.clear()
    rng = np.random.default_rng(5)
    many = rng.uniform(0.1, 1.0, size=(_lib.FRAY_MAX, S.m_lp))
    idx = F.push_batch(many)
    np.testing.assert_array_equal(idx, np.arange(_lib.FRAY_MAX))
    assert F.size == _lib.FRAY_MAX
    assert F.push_batch(3.0 * many[17:18])[0] == 17                       # a held ray still maps to its index
    with pytest.raises(TwoSDError) as e:
        F.push_batch(np.vstack([many[5:6], rng.uniform(0.1, 1.0, size=(1, S.m_lp))]))
    assert e.value.code == -5 and F.size == _lib.FRAY_MAX
    F.clear()
    assert F.size == 0
