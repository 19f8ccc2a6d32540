"""Writes tests/golden/lp_start_r07.npz: the decisions of storm LP batches in which every wave of
lp_hyper_kernel takes several scenarios in a row (tests/test_gpu_lp_start.py compares a build
against it bit for bit, under several launch shapes).  Run it on the GPU at the commit whose
arithmetic the fixture pins; a pull request that changes the arithmetic on purpose runs it again
and says so.
Usage: python tools/make_lp_start_golden.py [out.npz]

The existing fixture (tools/make_lp_paths_golden.py) pins the pivot paths, mostly at one scenario
per wave.  This one pins what a wave does between scenarios -- the claim of the next queue
position, its scenario and start basis, the start state, the epilogue's stores -- which only runs
when a wave solves several scenarios:
  batch   storm, pool of 256 bases with two-level candidates; the pool's 2048 training scenarios
          and their moved-element copies (4096 scenarios, the storm_pool case of the other tool)
          plus one more copy of scenario 0 (position 4096, for the N = 4097 edge)
  retry   the pivot-cap case of the other tool (pool of 16 under TWOSD_KMAX, cap and subset from
          its fixture), the subset laid out four times so that a wave takes several scenarios
The fixture is recorded at the default launch; the test solves the same batches under
TWOSD_BPC=1 (one block per CU: about four scenarios per wave at 4096) and TWOSD_QGROUPS=1 / 16.
Per scenario: status, pivots, objective, a digest of the pi row, the final pool pick; per batch the
keyed push (representatives, ordered V as row digests, fingerprint).  The keys themselves have no
accessor: they are pinned through the push, whose representatives are the first occurrences of
the keys and whose V is the representatives' pi rows in key order of appearance.
The batches and the per-batch run live here and are imported by the test, so the fixture and the
test cannot drift apart."""
import contextlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_lp_paths_golden as G  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "lp_start_r07.npz")
N_BATCH = 4096          # the batch proper; position 4096 repeats scenario 0
RETRY_COPIES = 4
KNOBS = ("TWOSD_BPC", "TWOSD_QGROUPS", "TWOSD_PUSH_MODE")


@contextlib.contextmanager
def launch_env(**env):
    """The launch knobs (read by the library at every launch) set for the block, all others unset."""
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in env.items():
            assert k in KNOBS, k
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def build_batch():
    """(ctx, x, epi, values): 4097 storm scenarios over a pool of 256 bases with candidates."""
    from sqlp_amd import twosd
    ctx, x, epi, vals = G.build_case("storm_pool")
    assert epi.num_scenarios == N_BATCH
    twosd.add_scenarios(epi, vals[:1])
    return ctx, x, epi, np.concatenate([vals, vals[:1]])


def build_retry():
    """(ctx, x, epi, values, primary ctx, primary epi): the capped case, RETRY_COPIES times over,
    and the same scenarios on a context without a pool."""
    from sqlp_amd import twosd
    gold = np.load(G.FIXTURE)
    cap, pool, subset = int(gold["storm_retry/cap"]), int(gold["storm_retry/pool"]), gold["storm_retry/subset"]
    ctx, x, epi, vals = G.build_case("storm_retry", (cap, pool, subset))
    for _ in range(RETRY_COPIES - 1):
        twosd.add_scenarios(epi, vals)
    allv = np.concatenate([vals] * RETRY_COPIES)
    # (without the cap: a start from the primary basis that stays within the cap is the same solve,
    # and the scenarios that only solve from their pool start are not compared)
    pctx, _, _ = G.new_ctx("storm")
    pepi = twosd.sdEpigraph(pctx, 1.0, 0.0)
    twosd.add_scenarios(pepi, allv)
    return ctx, x, epi, allv, pctx, pepi


def solve_range(ctx, x, epi, first, count, pool=True):
    """Lean and recovering solve of scenarios [first, first + count): per-scenario results."""
    from sqlp_amd import twosd
    out = {}
    obj, _, _, st = twosd.solve_batch(epi, x, first, count, want_pi=False)
    out["lean_obj"], out["lean_status"] = obj, st
    out["lean_pivots"] = ctx.last_lp_iters(count)[0]
    out["retries"] = np.int64(ctx.lp_counts()[1])
    if pool:
        out["lean_picks"] = np.asarray(ctx.last_pool_picks(count)).copy()
    obj, _, pi, st = twosd.solve_batch(epi, x, first, count, want_pi=True)
    out["full_obj"], out["full_status"] = obj, st
    out["full_pivots"] = ctx.last_lp_iters(count)[0]
    out["pi_digest"] = G.row_digests(pi)
    return out


def push_range(ctx, x, epi, first, count):
    """Keyed push of scenarios [first, first + count) into an empty V."""
    from sqlp_amd import twosd
    V = twosd.sdDualVertexSet(ctx)
    V.clear()
    obj, st, nv = twosd.solve_push(epi, x, first, count)
    return {"push_obj": obj, "push_status": st, "v_size": np.int64(nv),
            "v_digest": G.row_digests(V.matrix()) if nv else np.zeros(0, dtype=np.uint64),
            "v_fingerprint": np.uint64(V.fingerprint()), "push_reps": np.int64(ctx.last_push_reps()),
            "push_full": np.int64(ctx.last_push_mode())}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    data = {}
    ctx, x, epi, vals = build_batch()
    with launch_env(TWOSD_PUSH_MODE=1):
        res = solve_range(ctx, x, epi, 0, N_BATCH)
        res.update(push_range(ctx, x, epi, 0, N_BATCH))
    assert (res["lean_status"] == 0).all() and (res["full_status"] == 0).all() and (res["push_status"] == 0).all()
    assert (res["lean_pivots"] == res["full_pivots"]).all()
    assert res["lean_obj"].tobytes() == res["full_obj"].tobytes() == res["push_obj"].tobytes()
    piv = res["lean_pivots"]
    assert (piv == 0).any() and (piv == 1).any() and (piv >= 3).any(), "0, 1 and >= 3 pivots expected"
    for k, v in res.items():
        data[f"batch/{k}"] = v
    print(json.dumps({"case": "batch", "scenarios": int(len(piv)), "pivots_mean": float(piv.mean()), "pivots_0": int((piv == 0).sum()),
                      "pivots_1": int((piv == 1).sum()), "pivots_ge3": int((piv >= 3).sum()), "v_size": int(res["v_size"]),
                      "push_reps": int(res["push_reps"])}), flush=True)
    rctx, rx, repi, rvals, _, _ = build_retry()
    res = solve_range(rctx, rx, repi, 0, len(rvals))
    assert (res["lean_status"] == 0).all() and (res["full_status"] == 0).all()
    assert res["retries"] > 0
    for k, v in res.items():
        data[f"retry/{k}"] = v
    print(json.dumps({"case": "retry", "scenarios": int(len(rvals)), "retries": int(res["retries"]),
                      "pivots_max": int(res["lean_pivots"].max())}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **data)
    print(f"wrote {out_path}: {os.path.getsize(out_path)} bytes", flush=True)


if __name__ == "__main__":
    main()
