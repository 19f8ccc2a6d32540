"""Re-setting the template of a context (twosd_set_template on a handle that already holds one)
leaves the state of a fresh context: every device array of the old template is released with its
capacity, and statistics and heuristics start over.  The same calls on the same inputs are the
same code on the same data, so a re-used handle must give the bits of a fresh one.

lands and baa99-20 differ in m, n and k: lands -> baa99-20 grows every row length, the reverse
shrinks it, and the workload before the re-set uses as many scenarios as the one after it, so
every grow-only array is already large enough in rows (a capacity kept in rows of the old
template would skip an allocation the new template needs).

The last test creates and destroys a context many times and reads the device's free memory: a
device array that no destructor owns would lower it round after round."""
import numpy as np
import pytest

from tests import instances as I

pytestmark = pytest.mark.gpu

N = 256          # still below the max(N, 1024) floors of the per-scenario outputs
SEED = 20250219


def _workload(ctx, name, monkeypatch):
    """Basis, distributions, N sampled scenarios; a push in full mode and one in the default
    mode, a cut, and the stream moments.  Everything the comparison reads, by name."""
    from sqlp_amd import smps, twosd
    inst = I.load(name)
    x = I.x_ev(name)
    ctx.compute_basis(x, smps.mean_values(inst["sto"]))
    ctx.set_distributions(inst["sto"])
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, N, SEED)
    V = twosd.sdDualVertexSet(ctx)
    res = {}
    for tag, mode in (("full", "2"), ("auto", None)):
        if mode:
            monkeypatch.setenv("TWOSD_PUSH_MODE", mode)
        else:
            monkeypatch.delenv("TWOSD_PUSH_MODE", raising=False)
        V.clear()
        obj, st, size = twosd.solve_push(epi, x, 0, N)
        res[f"obj_{tag}"], res[f"status_{tag}"] = obj, st
        res[f"size_{tag}"] = np.array([size, len(V)])
        res[f"reps_{tag}"] = np.array([ctx.last_push_reps(), ctx.last_push_mode()])
    assert res["reps_full"][1] == 1          # the gathered-duals path ran
    res["V"] = V.matrix()
    cut = twosd.build_sasa_cut(epi, x, V)
    res["alpha"], res["beta"] = np.array([cut.alpha]), cut.beta
    m = twosd.evaluate_moments(ctx, np.zeros(len(x)), x, SEED + 1, 0, N)
    res["moments"] = np.array([m.n, m.n_bad, m.mean, m.m2, m.min, m.max], dtype=np.float64)
    return res


@pytest.mark.parametrize("first,second", [("lands", "baa99-20"), ("baa99-20", "lands")])
def test_reset_template_equals_fresh_context(first, second, monkeypatch):
    from sqlp_amd import twosd
    a, b = I.load(first), I.load(second)
    fresh = twosd.SDContext(b["sp2"], b["sto"])
    want = _workload(fresh, second, monkeypatch)
    fresh.close()
    assert (want["status_full"] == 0).all() and (want["status_auto"] == 0).all()

    ctx = twosd.SDContext(a["sp2"], a["sto"])
    _workload(ctx, first, monkeypatch)
    assert ctx.last_push_reps() > 0 and ctx.timings_us()[0] > 0      # there is something to forget
    ctx._set_problem(b["sp2"], b["sto"])
    # before any new call: the getters of a fresh context
    assert ctx.lp_stats() == (0, 0)
    assert ctx.last_push_reps() == 0 and ctx.last_push_mode() == 0
    assert ctx.lp_counts() == (0, 0)
    assert not np.any(ctx.timings_us()) and not np.any(ctx.last_refresh_ms())
    assert len(twosd.sdDualVertexSet(ctx)) == 0 and ctx.pool_size() == 0
    got = _workload(ctx, second, monkeypatch)
    ctx.close()
    assert set(got) == set(want)
    for key in sorted(want):
        assert got[key].shape == want[key].shape, key
        assert got[key].tobytes() == want[key].tobytes(), f"{key}: re-used handle differs from a fresh context"


def test_create_destroy_returns_device_memory():
    """50 contexts in a row, each with a template and one small solve.  The free memory after
    the last round may lie below the reading after the first by at most one round's footprint:
    the drop from before the first context to the moment before it is destroyed (measured, no
    constant).  A leak per round of the size of a context would come to 49 of them."""
    import torch
    from sqlp_amd import smps, twosd
    inst = I.load("lands")
    x = I.x_ev("lands")
    vals = I.sample("lands", 8, seed=3)

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    before = free_bytes()
    after_first = footprint = None
    for r in range(50):
        ctx = twosd.SDContext(inst["sp2"], inst["sto"])
        ctx.compute_basis(x, smps.mean_values(inst["sto"]))
        obj, _, _, st = ctx.solve_values(x, vals)
        assert (st == 0).all()
        if r == 0:
            footprint = before - free_bytes()
        ctx.close()
        if r == 0:
            after_first = free_bytes()
    after_last = free_bytes()
    print(f"free memory: before {before}, after round 1 {after_first}, after round 50 {after_last}; "
          f"one round's footprint {footprint}")
    assert footprint > 0
    assert after_first - after_last <= footprint
