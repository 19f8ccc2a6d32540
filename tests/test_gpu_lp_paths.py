"""The decisions of small LP batches that reach every path of lp_hyper_kernel, pinned bit for bit
against tests/golden/lp_paths_r06.npz (tools/make_lp_paths_golden.py, run at the commit whose
arithmetic the fixture holds; a change that alters the arithmetic on purpose regenerates it and
says so).

Cases (tools/make_lp_paths_golden.py builds and runs them, for the fixture and for this test):
  lands (R = 1), transship       every scenario from the primary basis
  ssn (R = 4, C = 14)            512 scenarios from the primary basis: ping-pong eta groups,
                                 Mask = uint32_t
  storm (R = 9, C = 28), primary 2048 device-sampled scenarios at x_EV: long solves (K well past
                                 2 EG, rows pivoted twice)
  storm, pool of 256 bases       two-level candidates; the batch is the pool's own 2048 training
                                 scenarios plus a copy of each with one element moved, so it holds
                                 solves of 0, 1 and >= 3 pivots (the K = 0 step alone, then the
                                 general path)
  storm, pivot cap               a pool of 16 under TWOSD_KMAX: some pool starts hit ITER_LIMIT and
                                 are retried from the primary basis
Each case runs the lean kernel (solve_batch without pi; solve_push with keys) and the recovering
kernel (solve_batch with pi) on the same scenarios.  Independently of the fixture every objective
is within 1e-9 relative of the C dual simplex of the oracle, as in tests/test_gpu_lp.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_lp_paths_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = list(G.CASES)


@pytest.fixture(scope="module")
def golden():
    return np.load(G.FIXTURE)


@pytest.fixture(scope="module")
def runs(golden):
    """Every case built and run once: case -> (results, x, scenario values)."""
    out = {}

    def get(case):
        if case not in out:
            retry = None
            if case == "storm_retry":
                retry = (int(golden["storm_retry/cap"]), int(golden["storm_retry/pool"]), golden["storm_retry/subset"])
            ctx, x, epi, vals = G.build_case(case, retry)
            out[case] = (G.run_case(ctx, x, epi), x, vals)
        return out[case]
    return get


def test_fixture_reaches_every_path(golden):
    piv = golden["storm_pool/lean_pivots"]
    assert (piv == 0).any() and (piv == 1).any() and (piv >= 3).any()
    assert golden["storm_retry/retries"] > 0
    assert golden["storm_primary/lean_pivots"].max() > 8        # K well past 2 EG
    for case in CASES:
        for k in ("lean_status", "full_status", "push_status"):
            assert (golden[f"{case}/{k}"] == 0).all(), (case, k)


@pytest.mark.parametrize("case", CASES)
def test_decisions_equal_fixture(case, golden, runs):
    res, _, _ = runs(case)
    for kernel in ("lean", "full"):
        np.testing.assert_array_equal(res[f"{kernel}_status"], golden[f"{case}/{kernel}_status"])
        np.testing.assert_array_equal(res[f"{kernel}_pivots"], golden[f"{case}/{kernel}_pivots"])
        # bit for bit: compared as integers (equal NaNs or signed zeros would not hide a change)
        np.testing.assert_array_equal(res[f"{kernel}_obj"].view(np.int64), golden[f"{case}/{kernel}_obj"].view(np.int64))
    assert int(res["retries"]) == int(golden[f"{case}/retries"])
    np.testing.assert_array_equal(res["pi_digest"], golden[f"{case}/pi_digest"])
    np.testing.assert_array_equal(res["push_status"], golden[f"{case}/push_status"])
    np.testing.assert_array_equal(res["push_obj"].view(np.int64), golden[f"{case}/push_obj"].view(np.int64))
    assert int(res["push_reps"]) == int(golden[f"{case}/push_reps"])
    assert int(res["v_size"]) == int(golden[f"{case}/v_size"])
    np.testing.assert_array_equal(res["v_digest"], golden[f"{case}/v_digest"])
    assert int(res["v_fingerprint"]) == int(golden[f"{case}/v_fingerprint"])


@pytest.fixture(scope="module")
def oracle_objectives():
    """C dual simplex objectives per scenario set (the three storm cases share one solve)."""
    from oracle import cpu
    cache = {}

    def get(name, x, vals):
        key = (name, vals.shape[0], vals.tobytes()[:4096])
        if key not in cache:
            sp2, sto, _ = G.load_instance(name)
            W, T = sp2.dense_W(), sp2.dense_T()
            lp = cpu.CpuLP(W, sp2.q, sp2.sense)
            ctx, _, _ = G.new_ctx(name)
            lp.set_basis(ctx.get_basis())
            obj, _, _, st, _ = lp.solve_batch(ctx.rows, sp2.r - T @ x, vals - sp2.r[ctx.rows], nthreads=8)
            assert (st == 0).all()
            cache[key] = obj
        return cache[key]
    return get


@pytest.mark.parametrize("case", CASES)
def test_objectives_match_oracle(case, runs, oracle_objectives):
    res, x, vals = runs(case)
    name = G.CASES[case][0]
    if case == "storm_retry":       # a subset of the storm scenarios: solved with them
        full = G.storm_values()
        sub = np.load(G.FIXTURE)["storm_retry/subset"]
        o_obj = oracle_objectives(name, x, full)[sub]
    else:
        o_obj = oracle_objectives(name, x, vals)
    for kernel in ("lean", "full", "push"):
        assert (res[f"{kernel}_status"] == 0).all()
        np.testing.assert_allclose(res[f"{kernel}_obj"], o_obj, rtol=1e-9, atol=1e-9)
