"""Writes tests/golden/lp_paths_r06.npz: the decisions of small LP batches that reach every path of
lp_hyper_kernel (tests/test_gpu_lp_paths.py compares a build against it bit for bit).  Run it on
the GPU at the commit whose arithmetic the fixture pins; a pull request that changes the
arithmetic on purpose runs it again and says so.
Usage: python tools/make_lp_paths_golden.py [out.npz]

Per case and scenario: status, pivots and objective of the lean kernel (solve_batch without pi)
and of the recovering kernel (solve_batch with pi), a 64-bit digest of every pi row, and the
ordered V of a keyed solve_push (rows as digests, plus its fingerprint).  Rows are kept as
digests (blake2b-8 of the row's bytes): equal digests <=> equal bits, at 8 bytes per row instead
of 8 m.  The case table and the per-case run live here (CASES, build_case, run_case) and are
imported by the test, so the fixture and the test cannot drift apart."""
import functools
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "lp_paths_r06.npz")
STORM_SEED = 20250701
# name -> (instance, scenarios, start)
CASES = {
    "lands": ("lands", 256, "primary"),
    "transship": ("transship", 256, "primary"),
    "ssn": ("ssn", 512, "primary"),
    "storm_primary": ("storm", 2048, "primary"),
    "storm_pool": ("storm", 2048, "pool256"),
    "storm_retry": ("storm", None, "capped"),      # a subset of the 2048, chosen by find_retry_case
}
RETRY_POOLS = (16, 8, 4, 2)


def row_digests(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.array([int.from_bytes(hashlib.blake2b(r.tobytes(), digest_size=8).digest(), "little") for r in a],
                    dtype=np.uint64)


def load_instance(name):
    from sqlp_amd import smps
    d = os.path.join(ROOT, "data", "smps", name)
    cor, tim, sto = smps.load_smps(d, name)
    sp2 = smps.get_smps_stage_template(cor, tim, 2)
    with open(os.path.join(ROOT, "tests", "golden", "ev_x.json")) as f:
        x = np.array(json.load(f)[name]["x"])
    return sp2, sto, x


def new_ctx(name, kmax=None):
    """Context at x_EV with the primary basis; kmax: the pivot cap (TWOSD_KMAX, read at creation)."""
    from sqlp_amd import smps, twosd
    sp2, sto, x = load_instance(name)
    old = os.environ.get("TWOSD_KMAX")
    if kmax is not None:
        os.environ["TWOSD_KMAX"] = str(int(kmax))
    try:
        ctx = twosd.SDContext(sp2, sto)
    finally:
        if kmax is not None:
            if old is None:
                del os.environ["TWOSD_KMAX"]
            else:
                os.environ["TWOSD_KMAX"] = old
    ctx.compute_basis(x, smps.mean_values(sto))
    return ctx, x, sto


@functools.lru_cache(maxsize=None)
def storm_values():
    """The 2048 device-sampled storm scenarios (element values) every storm case solves."""
    from sqlp_amd import twosd
    ctx, x, sto = new_ctx("storm")
    ctx.set_distributions(sto)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, 2048, STORM_SEED)
    return twosd.get_scenarios(epi, 0, 2048)


@functools.lru_cache(maxsize=None)
def storm_pool_heads(max_pool):
    """Heads of the pool_build pool of max_pool bases trained on the 2048 storm scenarios."""
    from sqlp_amd import twosd
    ctx, x, sto = new_ctx("storm")
    ctx.set_distributions(sto)
    tr = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(tr, 2048, STORM_SEED)
    size = ctx.pool_build(tr, x, 0, 2048, max_pool)
    return np.stack([ctx.pool_get(p) for p in range(size)])


def build_case(case, retry=None):
    """(ctx, x, epi, values) of a case.  retry = (cap, pool, subset) of the capped case."""
    from sqlp_amd import smps, twosd
    name, N, start = CASES[case]
    if start == "capped":
        cap, pool, subset = retry
        ctx, x, sto = new_ctx(name, kmax=cap)
        for h in storm_pool_heads(pool)[1:]:
            ctx.pool_add_basis(h)
        vals = storm_values()[np.asarray(subset)]
        epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
        twosd.add_scenarios(epi, vals)
        return ctx, x, epi, vals
    ctx, x, sto = new_ctx(name)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    if name == "storm":
        # the scenarios are drawn on the device; the pool trains on the batch itself, so the batch
        # holds every pool basis' own scenario (zero pivots) and its neighbours (one, a few)
        ctx.set_distributions(sto)
        twosd.add_sampled_scenarios(epi, N, STORM_SEED)
        if start == "pool256":
            assert ctx.pool_build(epi, x, 0, N, 256) > 32
            ctx.pool_build_candidates(epi, x, 0, N, 32, 16)
            # storm's sampled neighbours differ in many of the 117 elements and take two pivots or
            # more from the nearest pool basis, so the one-pivot solves (the K = 0 step alone) come
            # from a copy of every scenario with a single element moved to the next scenario's value
            base = twosd.get_scenarios(epi, 0, N)
            var = base.copy()
            e = (7 * np.arange(N)) % base.shape[1]
            var[np.arange(N), e] = np.roll(base, -1, axis=0)[np.arange(N), e]
            twosd.add_scenarios(epi, var)
        vals = twosd.get_scenarios(epi, 0, epi.num_scenarios)
    else:
        vals = smps.sample_values(sto, N, np.random.default_rng(7))
        twosd.add_scenarios(epi, vals)
    return ctx, x, epi, vals


def run_case(ctx, x, epi):
    """Lean solve, recovering solve and keyed push of the case's batch."""
    from sqlp_amd import twosd
    N = epi.num_scenarios
    out = {}
    obj, _, _, st = twosd.solve_batch(epi, x, 0, N, want_pi=False)          # lean kernel, no keys
    out["lean_obj"], out["lean_status"] = obj, st
    out["lean_pivots"] = ctx.last_lp_iters(N)[0]
    out["retries"] = np.int64(ctx.lp_counts()[1])
    obj, _, pi, st = twosd.solve_batch(epi, x, 0, N, want_pi=True)           # recovering kernel
    out["full_obj"], out["full_status"] = obj, st
    out["full_pivots"] = ctx.last_lp_iters(N)[0]
    out["pi_digest"] = row_digests(pi)
    V = twosd.sdDualVertexSet(ctx)
    V.clear()
    obj, st, nv = twosd.solve_push(epi, x, 0, N)                             # lean kernel with keys
    assert ctx.last_push_mode() == 0, "keyed push expected (the first push of a context)"
    out["push_obj"], out["push_status"] = obj, st
    out["v_size"] = np.int64(nv)
    out["v_digest"] = row_digests(V.matrix()) if nv else np.zeros(0, dtype=np.uint64)
    out["v_fingerprint"] = np.uint64(V.fingerprint())
    out["push_reps"] = np.int64(ctx.last_push_reps())
    return out


def find_retry_case(p0):
    """A pivot cap and a subset of the 2048 storm scenarios such that, from a small pool, some
    pool starts hit the cap and every scenario still solves (its pool start or its retry from the
    primary basis stays within the cap).  p0: pivots from the primary basis."""
    from sqlp_amd import twosd
    vals = storm_values()
    for pool in RETRY_POOLS:
        ctx, x, sto = new_ctx("storm")
        heads = storm_pool_heads(pool)
        for h in heads[1:]:
            ctx.pool_add_basis(h)
        epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
        twosd.add_scenarios(epi, vals)
        _, _, _, st = twosd.solve_batch(epi, x, 0, len(vals), want_pi=False)
        assert (st == 0).all()
        pp = ctx.last_lp_iters(len(vals))[0]
        picks = ctx.last_pool_picks(len(vals))
        worse = (pp > p0) & (picks > 0)
        print(f"retry search: pool {len(heads)}: {int(worse.sum())} pool starts take more pivots than the primary start",
              flush=True)
        if not worse.any():
            continue
        # the cap with the most retries
        best = max(range(int(p0[worse].min()), int(pp[worse].max())), key=lambda c: int(((p0 <= c) & (pp > c) & (picks > 0)).sum()))
        subset = np.nonzero(np.minimum(pp, p0) <= best)[0][:1024]
        keep = (p0[subset] <= best) & (pp[subset] > best) & (picks[subset] > 0)
        if keep.any():
            return best, pool, subset.astype(np.int32)
    raise SystemExit("no pivot cap separates a pool start from its primary start on these scenarios")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    data = {}
    retry = None
    for case in CASES:
        if case == "storm_retry":
            retry = find_retry_case(data["storm_primary/lean_pivots"])
            data["storm_retry/cap"] = np.int64(retry[0])
            data["storm_retry/pool"] = np.int64(retry[1])
            data["storm_retry/subset"] = retry[2]
        ctx, x, epi, vals = build_case(case, retry)
        res = run_case(ctx, x, epi)
        assert (res["lean_status"] == 0).all() and (res["full_status"] == 0).all() and (res["push_status"] == 0).all(), case
        assert (res["lean_pivots"] == res["full_pivots"]).all(), case
        assert res["lean_obj"].tobytes() == res["full_obj"].tobytes() == res["push_obj"].tobytes(), case
        for k, v in res.items():
            data[f"{case}/{k}"] = v
        piv = res["lean_pivots"]
        print(json.dumps({"case": case, "scenarios": int(len(piv)), "pivots_mean": float(piv.mean()), "pivots_max": int(piv.max()),
                          "pivots_0": int((piv == 0).sum()), "pivots_1": int((piv == 1).sum()), "pivots_ge3": int((piv >= 3).sum()),
                          "retries": int(res["retries"]), "v_size": int(res["v_size"]), "push_reps": int(res["push_reps"])}),
              flush=True)
    piv = data["storm_pool/lean_pivots"]
    assert (piv == 0).any() and (piv == 1).any() and (piv >= 3).any(), "storm_pool: 0, 1 and >= 3 pivots expected"
    assert data["storm_retry/retries"] > 0
    assert data["storm_primary/lean_pivots"].max() > 8
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **data)
    print(f"wrote {out_path}: {os.path.getsize(out_path)} bytes", flush=True)


if __name__ == "__main__":
    main()
