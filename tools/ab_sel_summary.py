"""Reduce an A/B of library builds (tools/ab_lp_builds.sh) for work on the warm-start selection: per
build and run the selection phase, the pool refresh (mean over the timed steps), the LP phase and the
step time; the gate against the first build (the parent) on each of them -- every run below every
parent run and the gain of the means >= 3 x the parent's spread -- and the result fields that must
equal the parent's.  The dumped outputs are compared by tools/ab_lp_summary.py or by checksum.
Usage: python tools/ab_sel_summary.py <session dir> <parent variant> <variant> [<variant> ...]"""
import glob
import json
import os
import sys

import numpy as np

SAME_TOP = ["lp_pivots_mean", "lp_pivots_max", "lp_iter_limit_retries"]
SAME_X = ["lp_pivots_mean", "lp_eta_entries", "push_representatives"]


def load(d, v):
    return [json.loads(open(f).read().strip().splitlines()[-1]) for f in sorted(glob.glob(os.path.join(d, f"bench_{v}_*.json")))]


def figures(r):
    steps = np.array([p["steps"] for p in r["x_points"]], dtype=float)
    refresh = np.array([p["pool_refresh_ms"] for p in r["x_points"]])
    return {"pool_select": r["phases_ms_per_step"]["pool_select"], "pool_refresh_ms": float((refresh * steps).sum() / steps.sum()),
            "lp_kernel": r["phases_ms_per_step"]["lp_kernel"], "ms_per_step": r["ms_per_step"]}


def main():
    d, variants = sys.argv[1], sys.argv[2:]
    runs = {v: load(d, v) for v in variants}
    fig = {v: [figures(r) for r in runs[v]] for v in variants}
    names = ["pool_select", "pool_refresh_ms", "lp_kernel", "ms_per_step"]
    for v in variants:
        print(f"== build {v}: {len(runs[v])} runs of bench.py --gpus 1 --steps 20 --warmup 5 (ms per step)")
        for i, f in enumerate(fig[v]):
            print(f"  run {i + 1}: " + "  ".join(f"{n} {f[n]:.3f}" for n in names))
        print("  mean : " + "  ".join(f"{n} {np.mean([f[n] for f in fig[v]]):.3f}" for n in names))
    parent = variants[0]
    print(f"== gate against {parent}: every run below every parent run, and gain of the means >= 3 x the parent's spread")
    for v in variants[1:]:
        for n in names:
            a, b = np.array([f[n] for f in fig[parent]]), np.array([f[n] for f in fig[v]])
            spread, gain, below = a.max() - a.min(), a.mean() - b.mean(), b.max() < a.min()
            verdict = "PASSED" if below and gain >= 3 * spread else "not passed"
            print(f"  {v} {n}: parent {a.mean():.3f} (spread {spread:.3f}) -> {b.mean():.3f}, gain {gain:.3f} ms "
                  f"({100 * gain / a.mean():.1f} %), all below: {below}, gate {verdict}")
    print("== same results as the parent")
    p0 = runs[parent][0]
    for v in variants[1:]:
        diffs = []
        for r in runs[v]:
            diffs += [k for k in SAME_TOP if r[k] != p0[k]]
            for xp, xq in zip(r["x_points"], p0["x_points"]):
                diffs += [f"x{xp['x']}:{k}" for k in SAME_X if xp[k] != xq[k]]
        print(f"  {v}: {'equal' if not diffs else 'DIFFERENT ' + str(sorted(set(diffs)))} ({', '.join(SAME_TOP + SAME_X)})")


if __name__ == "__main__":
    main()
