"""The mean-CVaR loop with its stopping rule (sqlp_amd/risk.py: sd_run_stop, bootstrap_gap_test) on
data/smps/lands3b at level 0.8 and lam 0.5, with the fixtures of tests/test_gpu_risk_loop.py: 60
iterations from lands' x_EV, one scenario per iteration (draws of seed 11), a check every 20
iterations with M = 16 replicates.

Bootstrap seed.  The host interior-point solver is known to stall on some replicates' degenerate
masters; the solver is not changed here.  The seed is the first of 5, 6, 7, 8 for
which all three checks run: 5.  Measured on all four: 5, 6 and 8 run the three checks (fractions
0 / 1 / 1, 0 / 0.9375 / 1, 0 / 0.875 / 0.9375 at eps 1e-3); 7 stalls at the first check (the master of
replicate 2 ends with ITERATION_LIMIT).

Tolerance: the project's cut tolerance 1e-8 (1 + |ref|) (tests/test_gpu_bootstrap._close)."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import boot_ref as BR
from tests.test_gpu_bootstrap import _close
from tests.test_gpu_risk_loop import LAM, draws, lands3b, recourse, risk_cell

pytestmark = pytest.mark.gpu

ITERS, EVERY, M, RUN_SEED = 60, 20, 16, 11
BOOT_SEED = 5         # the first of 5, 6, 7, 8 whose three checks all run (7 stalls: the docstring)


def _run(boot_seed, lam=LAM, iters=ITERS, **stop_args):
    """sd_run_stop with a stop that records every check and never passes."""
    from sqlp_amd import risk, twosd
    L = lands3b()
    ctx, cell = risk_cell(lam)
    d = draws(RUN_SEED, iters)
    checks = []

    def stop(c):
        res = risk.bootstrap_gap_test(c, M=M, seed=boot_seed, **stop_args)
        var, alpha, beta = c.master_rows()
        np.testing.assert_array_equal(res.rows0[0], var)
        _close(res.rows0[1], alpha, "row-0 master alpha")
        _close(res.rows0[2], beta, "row-0 master beta")
        assert res.gaps[0] >= -1e-8 * (1 + abs(res.U[0])), res.gaps[0]
        epi = c.cell.epi[0]
        assert twosd.picks_count(ctx) == len(epi.cuts) + len(c.tail_cuts) + 2      # no leak
        checks.append(SimpleNamespace(res=res, n=epi.num_scenarios, z=np.append(c.x_incumbent, c.eta_incumbent),
                                      zc=np.append(c.x_candidate, c.eta_candidate)))
        return SimpleNamespace(passed=False, res=res)
    it, last = risk.sd_run_stop(cell, lambda i: [L.support[d[i]][None, :]], iters, check_every=EVERY, stop=stop)
    assert it == iters and len(checks) == iters // EVERY and last.res is checks[-1].res
    return ctx, cell, d, checks


def test_loop_structure_and_determinism():
    ctx_a, _, _, a = _run(BOOT_SEED)
    ctx_a.close()
    ctx_b, _, _, b = _run(BOOT_SEED)
    ctx_b.close()
    assert len(a) == 3
    for ra, rb in zip(a, b):
        np.testing.assert_array_equal(ra.res.U, rb.res.U)
        np.testing.assert_array_equal(ra.res.L, rb.res.L)
        assert ra.res.fraction == rb.res.fraction and ra.res.passed == rb.res.passed
    print("RISK stop lands3b gaps at 20/40/60:", [float(r.res.gaps[0]) for r in a], "fractions", [r.res.fraction for r in a],
          "thresholds", [r.res.threshold for r in a])


def test_replicate_rows_bound_the_replicate_sample():
    """Every row of replicates 0..3 of the last check lies below the replicate's own empirical
    function -- sum c_s h_s / sum c_s for a mean row, sum c_s (h_s - eta)+ / sum c_s for a tail row,
    h by HiGHS, c the replicate's counts -- at the four (x, eta) points of
    test_mean_cvar_loop_on_lands3b."""
    L = lands3b()
    ctx, cell, d, checks = _run(BOOT_SEED)
    last = checks[-1]
    res = last.res
    assert len(res.rows) == M + 1 and last.n == ITERS
    x, eta = last.z[:-1], float(last.z[-1])
    points = [(x, eta), (last.zc[:-1], float(last.zc[-1])), (1.1 * x, eta - 25.0), (x + np.array([0.5, 0.0, 0.5, 0.0]), eta + 30.0)]
    cnt = BR.counts(BOOT_SEED, 0, ITERS, M)
    worst = -np.inf
    for b in range(4):
        c = np.ones(ITERS) if b == 0 else cnt[:, b - 1].astype(np.float64)
        assert c.sum() > 0
        var, alpha, beta = res.rows[b]
        assert (var == 0).sum() >= 2 and (var == 1).sum() >= 1
        for xp, ep in points:
            h = recourse(xp, L.support)[d]
            ref = (float(c @ h) / c.sum(), float(c @ np.maximum(h - ep, 0.0)) / c.sum())
            z = np.append(xp, ep)
            for v, a, be in zip(var, alpha, beta):
                row = a + float(be @ z)
                worst = max(worst, (row - ref[v]) / (1 + abs(ref[v])))
                assert row <= ref[v] + 1e-8 * (1 + abs(ref[v])), (b, v, row, ref[v], xp, ep)
    print(f"RISK stop lands3b: worst row excess over the replicates' empirical functions {worst:.2e} (relative)")
    ctx.close()


def test_loop_ends_when_the_test_passes():
    from sqlp_amd import risk
    L = lands3b()
    ctx, cell = risk_cell(LAM)
    d = draws(RUN_SEED, ITERS)
    it, res = risk.sd_run_stop(cell, lambda i: [L.support[d[i]][None, :]], ITERS, check_every=EVERY,
                               stop_args=dict(M=M, seed=BOOT_SEED, eps=1e9))
    assert it == EVERY and res.passed and res.fraction == 1.0
    ctx.close()


def test_lam_zero_is_the_risk_neutral_test():
    from sqlp_amd import risk, stopping
    L = lands3b()
    ctx, cell = risk_cell(0.0)
    d = draws(RUN_SEED, EVERY)
    for i in range(EVERY):
        risk.sd_iteration(cell, [L.support[d[i]][None, :]], keep_picks=True)
    a = risk.bootstrap_gap_test(cell, M=M, seed=BOOT_SEED)
    b = stopping.bootstrap_gap_test(cell.cell, M=M, seed=BOOT_SEED)
    np.testing.assert_array_equal(a.U, b.U)
    np.testing.assert_array_equal(a.L, b.L)
    ctx.close()
