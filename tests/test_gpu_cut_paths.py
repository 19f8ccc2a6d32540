"""The cut's two host paths give the same cut: twosd_build_cut against twosd_cut_partial +
twosd_cut_finalize (one driver, one epilogue each for timing, bookkeeping and the max_val / max_arg
copy), at shapes on the edges of the launch plan: (N, |V|) = (300, 40) whole tiles only, (1000, 256)
the tail split with the LDS histogram, (1000, 257) the tail split with the global histogram.

What other tests pin already and this one leaves to them: test_sharded_partials_equal_single_cut
(two shards + finalize against one build_cut: alpha / beta to 1e-12, the histogram bit-equal) and
test_tail_split_equals_whole_tiles (TWOSD_CUT_TAIL=0 against the split at 70k-100k scenarios:
max_arg / max_val equal, alpha / beta to 1e-13); parity with the oracle is test_gpu_cut.py's and
test_gpu_shapes.py's.  Here: bit equality of both paths' outputs on one epigraph, equal counters and
pass, the debug-scores call in between, the c0 shift of max_val, and the timing slots.

Instances: tests/synth_cases.synth_template (m2 = 40, k = 3 / 5 as in the plan table of
tests/test_cut_plan_host.py) with one non-random row i_z made inert (r = 0, T row = 0, so
(r - T x)[i_z] == 0 at every x).  The cut needs vertices, not LP duals: V is random vectors (of order 1
on the random rows, 0.05 elsewhere, and scenario values spread over +-4, so that many vertices win
scenarios), a quarter of them twice more as
- twins: copies that differ only in component i_z (the same PK row and the same base at every x:
  dropped from the argmax, or exact ties under TWOSD_CUT_TWINS=0), and
- near ties: copies moved along a direction that leaves the base unchanged up to rounding (where
  the rounded bases come out equal, such a copy is a dominated twin too: _dominated counts them in
  the cut's own arithmetic)."""
import ctypes as C

import numpy as np
import pytest

from tests import bounds_cases as BC
from tests import synth_cases as SC

pytestmark = pytest.mark.gpu
SHAPES = [(300, 40, 3), (1000, 256, 5), (1000, 257, 5)]
X = SC.X[0]
T_CUT_PARTIAL, T_CUT_FINALIZE = 2, 3


def _dominated(Vm, r, T, first_copy, n_orig_off):
    """The vertices the cut leaves out at X: copies (index >= first_copy, the copy of vertex
    v - n_orig_off) whose base equals their original's, the base as the cut forms it: T x summed
    from zero column by column, b = r - T x, then the products V[v][i] b[i] added in index order,
    every operation rounded on its own."""
    tx = np.zeros(len(r))
    for j in range(T.shape[1]):
        tx = tx + T[:, j] * X[j]
    b = r - tx
    base = np.zeros(len(Vm))
    for i in range(Vm.shape[1]):
        base = base + Vm[:, i] * b[i]
    return [v for v in range(first_copy, len(Vm)) if base[v] == base[v - n_orig_off]]


def _instance(N, nv, k, bounded=False):
    """(ctx, epi, S): a context over the template, V of exactly nv vertices, an epigraph of N
    weighted scenarios; S.dropped: the vertices the argmax leaves out.  bounded: lower bounds 0.25
    on the six dearest columns (c0 = q . lb = 75)."""
    from sqlp_amd import twosd
    S = SC.synth_template(40, 128, k, seed=31 + k)
    r, T = S.r.copy(), S.T.copy()
    quiet = [i for i in range(S.m2) if i not in set(S.rows.tolist())]
    iz, i1, i2 = quiet[:3]
    r[iz] = 0.0
    T[iz, :] = 0.0
    lb, ub = S.lb.copy(), S.ub.copy()
    if bounded:
        lb[np.argsort(-S.q)[:6]] = 0.25
    ctx = twosd.SDContext(BC.stage_problem(S.W, T, S.q, r, S.sense, lb, ub), positions=S.positions)
    assert ctx.k == k
    m = ctx.mv
    rng = np.random.default_rng(7)
    n_twin = n_near = nv // 4                        # vertices [0, n) have a twin, [n, 2 n) a near tie
    base = 0.05 * rng.uniform(-1.0, 1.0, size=(nv - n_twin - n_near, m))
    base[:, S.rows] = rng.uniform(-1.0, 1.0, size=(len(base), k))
    twins = base[:n_twin].copy()
    twins[:, iz] += 1.0
    b = (r - S.W @ lb) - T @ X                       # the canonical r - T x (lower bounds only: no bound rows)
    near = base[n_twin:n_twin + n_near].copy()
    near[:, i1] += 0.5
    near[:, i2] -= 0.5 * b[i1] / b[i2]
    V = twosd.sdDualVertexSet(ctx)
    Vm = np.vstack([base, twins, near])
    V.push_batch(Vm)
    assert len(V) == nv
    S.dropped = None if bounded else _dominated(Vm, r, T, len(base), len(base))
    assert bounded or S.dropped[:n_twin] == list(range(len(base), len(base) + n_twin))    # every twin, and maybe near ties
    vals = r[S.rows] + np.random.default_rng(11).uniform(-4.0, 4.0, size=(N, k))
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals, np.random.default_rng(5).uniform(0.5, 1.5, size=N))
    S.r_user, S.T_user, S.lb_user, S.vals, S.n_copy = r, T, lb, vals, n_twin
    return ctx, epi, S


def _state(ctx):
    return dict(stats=ctx.cut_stats(), cut_pass=ctx.cut_pass(), kind=ctx.cut_pass_kind())


def _build(ctx, epi, tie_rel):
    from sqlp_amd import twosd
    cut, mv, ma = twosd._build_cut(epi, X, tie_rel, want_argmax=True)
    return dict(alpha=cut.alpha, beta=cut.beta, mv=mv, ma=ma, **_state(ctx))


def _split(ctx, epi, tie_rel, between=None):
    """twosd_cut_partial (with max_val / max_arg) + twosd_cut_finalize on device buffers."""
    import torch
    from sqlp_amd._lib import check, ptr
    nu, nf = ctx.cut_partial_len()
    dev = torch.device("cuda", 0)
    hist = torch.zeros(nu, dtype=torch.int64, device=dev)
    sums = torch.zeros(nf, dtype=torch.float64, device=dev)
    N = epi.num_scenarios
    mv, ma = np.zeros(N), np.zeros(N, dtype=np.int32)
    x = np.ascontiguousarray(X, dtype=np.float64)
    check(ctx.lib.twosd_cut_partial(ctx.h, epi.index, ptr(x), float(tie_rel), float(epi.total_scenario_weight),
                                    C.c_void_p(hist.data_ptr()), C.c_void_p(sums.data_ptr()), ptr(mv), ptr(ma)))
    st = _state(ctx)
    if between:
        between()
    a, b = ctx.cut_finalize(X, hist.data_ptr(), sums.data_ptr())
    return dict(alpha=a, beta=b, mv=mv, ma=ma, **st)


def _assert_same(p, q, what):
    for key in p:
        same = np.array_equal(p[key], q[key]) if isinstance(p[key], np.ndarray) else p[key] == q[key]
        assert same, (what, key, p[key], q[key])


@pytest.mark.parametrize("N,nv,k", SHAPES)
@pytest.mark.parametrize("twins", ["1", "0"])
def test_build_cut_equals_partial_plus_finalize(N, nv, k, twins, monkeypatch):
    monkeypatch.setenv("TWOSD_CUT_TWINS", twins)
    ctx, epi, S = _instance(N, nv, k)
    assert (ctx.timings_us()[[T_CUT_PARTIAL, T_CUT_FINALIZE]] == 0.0).all()

    def after_partial():
        t = ctx.timings_us()
        assert t[T_CUT_PARTIAL] > 0.0 and t[T_CUT_FINALIZE] == 0.0, t

    for tie_rel in (0.0, 1e-12):
        two = _split(ctx, epi, tie_rel, between=after_partial if tie_rel == 0.0 else None)
        assert ctx.timings_us()[T_CUT_FINALIZE] > 0.0
        one = _build(ctx, epi, tie_rel)
        print(f"CUTPATHS N {N} |V| {nv} twins {twins} tie_rel {tie_rel}: alpha {one['alpha']!r} stats {one['stats']} "
              f"pass {one['cut_pass']} kind {one['kind']} timings {ctx.timings_us()[[T_CUT_PARTIAL, T_CUT_FINALIZE]]}")
        _assert_same(one, two, (N, nv, twins, tie_rel))
        assert (ctx.timings_us()[[T_CUT_PARTIAL, T_CUT_FINALIZE]] > 0.0).all()
        assert one["ma"].min() >= 0 and one["ma"].max() < nv
        n, ma = S.n_copy, one["ma"]
        assert len(np.unique(ma)) >= 8                         # the scenarios spread over the vertices
        # a twin never wins: its original, lower in the set, has the same restated score for every
        # scenario, and both rules take the lower index (a near tie may win: its score differs by rounding)
        assert not ((ma >= nv - 2 * n) & (ma < nv - n)).any()
        if twins == "1":
            assert one["stats"][3] == len(S.dropped)           # every twin is dominated at every x
            # a scenario won by a vertex whose near tie stays in the argmax has two vertices in the band
            kept = [v for v in range(n, 2 * n) if v + (nv - 2 * n) not in S.dropped]
            assert one["stats"][0] >= np.isin(ma, kept).sum()
        else:
            # nothing left out: a scenario won by a vertex with a twin or a near tie is re-decided
            assert one["stats"][3] == 0 and N >= one["stats"][0] >= (ma < 2 * n).sum() > 0
            if nv == 2 * (nv - 2 * n):                         # every original has a copy: every scenario
                assert one["stats"][0] == N


def test_tail_split_off_both_paths(monkeypatch):
    """(1000, 256): TWOSD_CUT_TAIL=0 (whole tiles, no merge kernel) against unset (two vertex ranges per
    tail tile).  Both paths agree bit for bit under either setting; between the settings the picks
    and their values are the same bits, and alpha / beta, whose sums run over other partial slots,
    agree to 1e-13 (N u = 1.1e-13 for the N = 1000 reordered fp64 terms; the bound that
    test_tail_split_equals_whole_tiles holds at 70k-100k scenarios)."""
    ctx, epi, S = _instance(1000, 256, 5)
    res = {}
    for tail in (None, "0"):
        if tail is None:
            monkeypatch.delenv("TWOSD_CUT_TAIL", raising=False)
        else:
            monkeypatch.setenv("TWOSD_CUT_TAIL", tail)
        one, two = _build(ctx, epi, 1e-12), _split(ctx, epi, 1e-12)
        _assert_same(one, two, ("tail", tail))
        res[tail] = one
        print(f"CUTPATHS tail {tail}: alpha {one['alpha']!r} stats {one['stats']} pass {one['cut_pass']}")
    on, off = res[None], res["0"]
    np.testing.assert_array_equal(on["ma"], off["ma"])
    np.testing.assert_array_equal(on["mv"], off["mv"])
    assert on["cut_pass"] == off["cut_pass"] and on["kind"] == off["kind"] and on["stats"][3] == off["stats"][3]
    assert on["alpha"] == pytest.approx(off["alpha"], rel=1e-13, abs=1e-13)
    np.testing.assert_allclose(on["beta"], off["beta"], rtol=1e-13, atol=1e-13)


def test_debug_scores_between_two_cuts():
    """twosd_cut_debug_scores runs a cut of its own (tie_rel 0) on the shared workspace: the cut after
    it equals the cut before it, outputs and counters."""
    ctx, epi, S = _instance(1000, 256, 5)
    first = _build(ctx, epi, 1e-12)
    assert first["kind"][0] == 2                               # the integer pass: the scores exist
    t, vmap = ctx.cut_debug_scores(epi.index, X, 1000, 256)
    assert vmap.tolist() == [v for v in range(256) if v not in S.dropped] and len(vmap) <= 256 - 64   # all but the dominated twins
    assert t.shape == (1000, len(vmap)) and np.isfinite(t).all()
    second = _build(ctx, epi, 1e-12)
    _assert_same(first, second, "debug scores in between")
    _assert_same(first, _split(ctx, epi, 1e-12), "debug scores before the split path")


def test_max_val_carries_the_shift_on_both_paths():
    """General bounds (lower bounds on six columns): max_val is the caller's objective, the
    canonical LP's score plus c0 = q . lb, from twosd_build_cut and from twosd_cut_partial."""
    ctx, epi, S = _instance(300, 40, 3, bounded=True)
    from sqlp_amd import twosd
    c0 = float(S.q @ S.lb_user)
    assert c0 == 75.0                                          # six penalty columns: far above the comparison's tolerance
    one, two = _build(ctx, epi, 0.0), _split(ctx, epi, 0.0)
    _assert_same(one, two, "bounded")
    Vm = twosd.sdDualVertexSet(ctx).matrix()
    assert Vm.shape[1] == S.m2                                 # lower bounds add no rows
    scores = (Vm @ ((S.r_user - S.W @ S.lb_user) - S.T_user @ X))[None, :] + (S.vals - S.r_user[S.rows]) @ Vm[:, S.rows].T
    print("CUTPATHS bounded c0", c0, "max |mv - (score + c0)|", np.abs(one["mv"] - (scores.max(1) + c0)).max())
    np.testing.assert_allclose(one["mv"], scores.max(1) + c0, rtol=1e-10, atol=1e-9)
    assert np.abs(one["mv"] - scores.max(1)).min() > 0.5 * c0  # and not the unshifted score
