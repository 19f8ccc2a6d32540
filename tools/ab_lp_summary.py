"""Reduce an A/B of library builds (tools/ab_lp_builds.sh) to the round's summary: per build and run
the LP time per step, step time and throughput, per x point LP ms and mean pivots, the least-squares
line of LP ms against mean pivots over the x points, the gate against the first build (the parent:
every run below every parent run, gain of the means >= 3 x the parent's spread), the result fields
that must equal the parent's, and the byte comparison of the dumped outputs.
Usage: python tools/ab_lp_summary.py <session dir> <parent variant> <variant> [<variant> ...]"""
import glob
import json
import os
import sys

import numpy as np

SAME_TOP = ["lp_pivots_mean", "lp_pivots_max", "lp_iter_limit_retries"]
SAME_X = ["lp_pivots_mean", "lp_eta_entries", "push_representatives"]
DUMPS = ["cut_alpha", "cut_beta", "objective_sums", "new_vertices"]


def load(d, v):
    runs = []
    for f in sorted(glob.glob(os.path.join(d, f"bench_{v}_*.json"))):
        runs.append((f, json.loads(open(f).read().strip().splitlines()[-1])))
    return runs


def line_fit(r):
    piv = np.array([p["lp_pivots_mean"] for p in r["x_points"]])
    ms = np.array([p["lp_kernel_ms"] for p in r["x_points"]])
    slope, icpt = np.polyfit(piv, ms, 1)
    return slope, icpt


def main():
    d, variants = sys.argv[1], sys.argv[2:]
    data = {v: load(d, v) for v in variants}
    parent = variants[0]
    lp = {v: np.array([r["phases_ms_per_step"]["lp_kernel"] for _, r in data[v]]) for v in variants}
    for v in variants:
        print(f"== build {v}: {len(data[v])} runs of bench.py --gpus 1 --steps 20 --warmup 5")
        for f, r in data[v]:
            s, i = line_fit(r)
            xs = " ".join(f"[lp {p['lp_kernel_ms']:.2f} ms piv {p['lp_pivots_mean']:.4f}]" for p in r["x_points"])
            print(f"  {os.path.basename(f)}: lp_kernel {r['phases_ms_per_step']['lp_kernel']:.3f} ms  ms_per_step {r['ms_per_step']:.3f}  "
                  f"value {r['value']:.0f}  | {xs} | fit {s:.3f} ms/pivot + {i:.2f} ms")
        fits = np.array([line_fit(r) for _, r in data[v]])
        print(f"  lp_kernel mean {lp[v].mean():.3f} ms, min {lp[v].min():.3f}, max {lp[v].max():.3f}, spread {lp[v].max() - lp[v].min():.3f}; "
              f"fit mean {fits[:, 0].mean():.3f} ms per pivot per 1M + {fits[:, 1].mean():.2f} ms")
    spread = lp[parent].max() - lp[parent].min()
    print(f"== gate against {parent} (spread of its runs {spread:.3f} ms; a gain counts from {3 * spread:.3f} ms)")
    p0 = data[parent][0][1]
    for v in variants[1:]:
        gain = lp[parent].mean() - lp[v].mean()
        below = lp[v].max() < lp[parent].min()
        ok = below and gain >= 3 * spread
        print(f"  {v}: gain of the means {gain:.3f} ms ({100 * gain / lp[parent].mean():.1f} %), every run below every parent run: {below}, "
              f"gate {'PASSED' if ok else 'not passed'}")
    print("== same results as the parent")
    for v in variants[1:]:
        diffs = []
        for _, r in data[v]:
            diffs += [k for k in SAME_TOP if r.get(k) != p0.get(k)]
            for px, qx in zip(r["x_points"], p0["x_points"]):
                diffs += [k for k in SAME_X if px.get(k) != qx.get(k)]
        print(f"  {v}: bench fields {SAME_TOP + SAME_X}: {'equal' if not diffs else 'DIFFER ' + str(sorted(set(diffs)))}")
        pd = sorted(glob.glob(os.path.join(d, f"dump_{parent}_*")))[0]
        for dd in sorted(glob.glob(os.path.join(d, f"dump_{v}_*"))):
            res = []
            for name in DUMPS:
                a, b = os.path.join(pd, name + ".npy"), os.path.join(dd, name + ".npy")
                res.append(f"{name} {'equal' if open(a, 'rb').read() == open(b, 'rb').read() else 'DIFFERS'}")
            print(f"  {os.path.basename(dd)} vs {os.path.basename(pd)}: " + ", ".join(res))


if __name__ == "__main__":
    main()
