"""What a wave of lp_hyper_kernel does between scenarios -- the claim of the next queue position, its
record (scenario, start basis), the start state, the epilogue's stores -- under launch shapes in
which a wave takes several scenarios in a row, pinned bit for bit against
tests/golden/lp_start_r07.npz (tools/make_lp_start_golden.py, which builds the batches for the
fixture and for this test; the fixture is recorded at the default launch).

No scenario's arithmetic depends on which wave runs it or in what order, so every launch shape
gives the fixture's status, pivots, objective bits, pi rows and keyed push.  (The keys have no
accessor; they are pinned through the push: its representatives are the first occurrences of the
keys, V is their pi rows in order of appearance.)

Shapes: TWOSD_BPC=1 is one 4-wave block per CU (1024 waves: about four scenarios per wave at
4096), TWOSD_QGROUPS the number of queue ranges.  The library never cuts an empty range (ranges
<= blocks <= ceil(N / 4), so every range holds a position); what does happen is a wave that finds
its ranges emptied by others before its first claim, or after its only scenario: N = 64 under
TWOSD_BPC=1 gives every wave one scenario and an exhausted queue behind it, N = 67 puts two
blocks on one range of four positions, so four waves never get a scenario."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_lp_paths_golden as G  # noqa: E402
import make_lp_start_golden as S  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {
    "default": {},
    "bpc1": {"TWOSD_BPC": 1},
    "qgroups1": {"TWOSD_QGROUPS": 1},
    "qgroups16": {"TWOSD_QGROUPS": 16},
    "bpc1_qgroups1": {"TWOSD_BPC": 1, "TWOSD_QGROUPS": 1},
    "bpc1_qgroups16": {"TWOSD_BPC": 1, "TWOSD_QGROUPS": 16},
}
PER_SCENARIO = ("lean_status", "lean_pivots", "lean_obj", "lean_picks", "full_status", "full_pivots", "full_obj", "pi_digest")


def bits(a):
    """Compared as integers: equal NaNs or signed zeros would not hide a change."""
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_same(res, ref, keys, sel=None, what=""):
    for k in keys:
        r = ref[k] if sel is None else ref[k][sel]
        np.testing.assert_array_equal(bits(res[k]), bits(r), err_msg=f"{what}: {k}")


@pytest.fixture(scope="module")
def golden():
    return np.load(S.FIXTURE)


@pytest.fixture(scope="module")
def batch():
    return S.build_batch()


@pytest.fixture(scope="module")
def batch_ref(golden):
    return {k: golden[f"batch/{k}"] for k in PER_SCENARIO + ("push_obj", "push_status", "v_digest", "v_fingerprint", "push_reps", "v_size")}


def test_fixture_holds_short_and_long_solves(golden):
    piv = golden["batch/lean_pivots"]
    assert len(piv) == S.N_BATCH
    assert (piv == 0).any() and (piv == 1).any() and (piv >= 3).any()
    assert (golden["batch/lean_status"] == 0).all() and (golden["batch/full_status"] == 0).all()
    assert golden["retry/retries"] > 0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_shape_invariance(shape, batch, batch_ref):
    ctx, x, epi, _ = batch
    with S.launch_env(TWOSD_PUSH_MODE=1, **SHAPES[shape]):
        res = S.solve_range(ctx, x, epi, 0, S.N_BATCH)
        res.update(S.push_range(ctx, x, epi, 0, S.N_BATCH))
    piv = res["lean_pivots"]
    assert (piv == 0).any() and (piv == 1).any() and (piv >= 3).any()
    assert_same(res, batch_ref, PER_SCENARIO + ("push_obj", "push_status", "v_digest"), what=shape)
    assert int(res["push_reps"]) == int(batch_ref["push_reps"])
    assert int(res["v_size"]) == int(batch_ref["v_size"])
    assert int(res["v_fingerprint"]) == int(batch_ref["v_fingerprint"])


def test_objectives_match_oracle(batch, batch_ref):
    from oracle import cpu
    _, x, _, vals = batch
    sp2, _, _ = G.load_instance("storm")
    lp = cpu.CpuLP(sp2.dense_W(), sp2.q, sp2.sense)
    pctx, _, _ = G.new_ctx("storm")
    lp.set_basis(pctx.get_basis())
    o_obj, _, _, st, _ = lp.solve_batch(pctx.rows, sp2.r - sp2.dense_T() @ x, vals[:S.N_BATCH] - sp2.r[pctx.rows], nthreads=8)
    assert (st == 0).all()
    for k in ("lean_obj", "full_obj", "push_obj"):
        np.testing.assert_allclose(batch_ref[k], o_obj, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("N", [1, 3, 64, 67, 4097])
def test_queue_edges(N, batch, batch_ref):
    """The first N scenarios under TWOSD_BPC=1 against the same scenarios of the 4096-batch
    (position 4096 repeats scenario 0)."""
    ctx, x, epi, _ = batch
    sel = np.arange(N) % S.N_BATCH
    with S.launch_env(TWOSD_BPC=1):
        res = S.solve_range(ctx, x, epi, 0, N)
    assert_same(res, batch_ref, PER_SCENARIO, sel=sel, what=f"N={N}")


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("bpc", [None, 1])
def test_push_modes(mode, bpc, batch, batch_ref):
    """Mode 1 re-solves the representatives through the list (pi by position), mode 2 recovers every
    dual in the main pass (the full kernel with keys): the same V and representatives."""
    ctx, x, epi, _ = batch
    env = {"TWOSD_PUSH_MODE": mode}
    if bpc:
        env["TWOSD_BPC"] = bpc
    with S.launch_env(**env):
        res = S.push_range(ctx, x, epi, 0, S.N_BATCH)
    assert int(res["push_full"]) == (1 if mode == 2 else 0)
    assert_same(res, batch_ref, ("push_obj", "push_status", "v_digest"), what=f"mode {mode}")
    assert int(res["push_reps"]) == int(batch_ref["push_reps"])
    assert int(res["v_fingerprint"]) == int(batch_ref["v_fingerprint"])


def test_retry_with_several_scenarios_per_wave(golden):
    """Pool starts that hit the pivot cap are solved again from the primary basis while the next
    scenario's prefetched record waits: every scenario that ends with pick 0 equals its solve on a
    context without a pool, and the whole batch equals the fixture."""
    ctx, x, epi, vals, pctx, pepi = S.build_retry()
    N = len(vals)
    ref = {k: golden[f"retry/{k}"] for k in PER_SCENARIO}
    cap = int(np.load(G.FIXTURE)["storm_retry/cap"])
    with S.launch_env():
        prim = S.solve_range(pctx, x, pepi, 0, N, pool=False)
    for shape in ({}, {"TWOSD_BPC": 1}, {"TWOSD_BPC": 1, "TWOSD_QGROUPS": 1}):
        with S.launch_env(**shape):
            res = S.solve_range(ctx, x, epi, 0, N)
        assert int(res["retries"]) == int(golden["retry/retries"]) > 0
        assert_same(res, ref, PER_SCENARIO, what=f"retry {shape}")
        back = res["lean_picks"] == 0            # started from, or retried from, the primary basis
        assert back.sum() >= int(res["retries"])
        for k in ("lean_status", "lean_obj", "full_status", "full_obj", "pi_digest"):
            np.testing.assert_array_equal(bits(res[k])[back], bits(prim[k])[back], err_msg=f"retry {shape}: {k}")
        # the pivot count of a retried scenario includes the capped attempt: cap + its primary solve
        for k in ("lean_pivots", "full_pivots"):
            extra = res[k][back] - prim[k][back]
            assert np.isin(extra, (0, cap)).all(), f"retry {shape}: {k}"
            assert int((extra == cap).sum()) == int(res["retries"]), f"retry {shape}: {k}"


@pytest.mark.parametrize("name", ["lands", "transship"])
def test_no_pool_no_order(name):
    """Neither a pool nor an order (the kernel reads no record): 4097 scenarios from the primary
    basis under TWOSD_BPC=1 against the default launch."""
    from sqlp_amd import smps, twosd
    ctx, x, sto = G.new_ctx(name)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, smps.sample_values(sto, 4097, np.random.default_rng(7)))
    keys = tuple(k for k in PER_SCENARIO if k != "lean_picks")
    with S.launch_env():
        ref = S.solve_range(ctx, x, epi, 0, 4097, pool=False)
    assert (ref["lean_status"] == 0).all() and (ref["full_status"] == 0).all()
    for shape in ({"TWOSD_BPC": 1}, {"TWOSD_BPC": 1, "TWOSD_QGROUPS": 1}):
        with S.launch_env(**shape):
            res = S.solve_range(ctx, x, epi, 0, 4097, pool=False)
        assert_same(res, ref, keys, what=f"{name} {shape}")
