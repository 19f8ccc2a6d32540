"""The record of the last LP batch after twosd_solve_push (LpBatchRecord, twosd_ctx.h).

A push solves its batch once (the main pass) and then, in re-solve mode, launches the LP kernel a
second time over the representatives only.  The twosd_last_* getters describe the batch: pivot sum
and maximum, eta entries, retries, the weighted objective sums and the pool picks are those of
the main pass whichever way the duals reach V -- every dual pushed (TWOSD_PUSH_ALL=1), the
representatives re-solved (TWOSD_PUSH_MODE=1) or gathered from the main pass (TWOSD_PUSH_MODE=2)
-- and they are what a plain solve_batch of the same scenarios reports.  The FMA count
(twosd_last_lp_ops) is left out: recovering every dual costs FMAs the keyed pass does not spend."""
import numpy as np
import pytest

from tests import instances as I

pytestmark = pytest.mark.gpu

MODES = (("all", {"TWOSD_PUSH_ALL": "1", "TWOSD_PUSH_MODE": "0"}),
         ("resolve", {"TWOSD_PUSH_ALL": "0", "TWOSD_PUSH_MODE": "1"}),
         ("full", {"TWOSD_PUSH_ALL": "0", "TWOSD_PUSH_MODE": "2"}))


def _record(ctx, N):
    return dict(lp_stats=ctx.lp_stats(), lp_counts=ctx.lp_counts(), objective=ctx.last_objective(),
                picks=ctx.last_pool_picks(N))


# storm: a pool of 16 from 256 training scenarios, so the selection runs and the keyed push meets
# shared vertices; lands: the primary basis alone (no pool, no queue records), few representatives
@pytest.mark.parametrize("name,N,train,pool", [("storm", 2048, 256, 16), ("lands", 256, 0, 1)])
def test_push_leaves_the_batch_record(name, N, train, pool, monkeypatch):
    from sqlp_amd import smps, twosd
    inst = I.load(name)
    ctx = twosd.SDContext(inst["sp2"], inst["sto"])
    x = I.x_ev(name)
    ctx.compute_basis(x, smps.mean_values(inst["sto"]))
    if pool > 1:
        tr = twosd.sdEpigraph(ctx, 1.0, 0.0)
        twosd.add_scenarios(tr, I.sample(name, train, seed=5))
        assert 1 < ctx.pool_build(tr, x, 0, train, pool) <= pool
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, I.sample(name, N, seed=17))
    V = twosd.sdDualVertexSet(ctx)

    obj_b, _, _, st_b = twosd.solve_batch(epi, x, 0, N, want_pi=False)
    assert (st_b == 0).all()
    batch = _record(ctx, N)
    print(f"{name} solve_batch: {batch['lp_stats']} {batch['lp_counts']} {batch['objective']}")

    runs = {}
    for tag, env in MODES:
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        V.clear()
        obj, st, _ = twosd.solve_push(epi, x, 0, N)
        assert (st == 0).all()
        np.testing.assert_array_equal(obj, obj_b)
        runs[tag] = _record(ctx, N)
        t = ctx.timings_us()
        reps, full = ctx.last_push_reps(), ctx.last_push_mode()
        print(f"{name} push {tag}: {runs[tag]['lp_stats']} {runs[tag]['lp_counts']} {runs[tag]['objective']} "
              f"reps {reps} full {full} lp {t[0]:.1f} us select {t[4]:.1f} us")
        assert t[0] > 0
        assert full == (1 if tag == "full" else 0)
        assert reps == N if tag == "all" else 0 < reps < N      # resolve: the second launch ran
    ctx.close()

    for tag, _ in MODES:
        got = runs[tag]
        assert got["lp_stats"] == runs["all"]["lp_stats"], tag
        assert got["lp_counts"] == runs["all"]["lp_counts"], tag
        assert got["objective"] == runs["all"]["objective"], tag
        np.testing.assert_array_equal(got["picks"], runs["all"]["picks"])
        assert got["lp_stats"] == batch["lp_stats"], tag
        assert got["objective"] == batch["objective"], tag
    if pool > 1:
        assert len(np.unique(runs["all"]["picks"])) > 1          # the selection chose among the pool
    else:
        assert not runs["all"]["picks"].any()
