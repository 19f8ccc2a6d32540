"""Reduce an A/B of library builds (tools/ab_lp_builds.sh) for a change of the cut: per build and
run the cut_partial phase and the step, the gate against the first build (the parent: every run
below every parent run, gain of the means >= 3 x the parent's spread) on both, the re-decided row
counts, and the dumped outputs against the parent's (byte-equal, or the largest difference).
Usage: python tools/ab_cut_summary.py <session dir> <parent variant> <variant> [<variant> ...]"""
import glob
import json
import os
import sys

import numpy as np

DUMPS = ["cut_alpha", "cut_beta", "objective_sums", "new_vertices"]


def load(d, v):
    return [(f, json.loads(open(f).read().strip().splitlines()[-1])) for f in sorted(glob.glob(os.path.join(d, f"bench_{v}_*.json")))]


def gate(name, a, b):
    spread = a.max() - a.min()
    gain = a.mean() - b.mean()
    below = b.max() < a.min()
    ok = below and gain >= 3 * spread
    return (f"{name}: parent mean {a.mean():.3f} ms (spread {spread:.3f}), build mean {b.mean():.3f} ms (min {b.min():.3f}, max {b.max():.3f}); "
            f"gain {gain:.3f} ms ({100 * gain / a.mean():.1f} %), every run below every parent run: {below}, gate {'PASSED' if ok else 'not passed'}")


def main():
    d, variants = sys.argv[1], sys.argv[2:]
    data = {v: load(d, v) for v in variants}
    parent = variants[0]
    cut = {v: np.array([r["phases_ms_per_step"]["cut_partial"] for _, r in data[v]]) for v in variants}
    step = {v: np.array([r["ms_per_step"] for _, r in data[v]]) for v in variants}
    for v in variants:
        print(f"== build {v}: {len(data[v])} runs")
        for f, r in data[v]:
            ph = r["phases_ms_per_step"]
            print(f"  {os.path.basename(f)}: cut_partial {ph['cut_partial']:.3f} ms  lp_kernel {ph['lp_kernel']:.3f}  pool_select {ph['pool_select']:.3f}  "
                  f"ms_per_step {r['ms_per_step']:.3f}  value {r['value']:.0f}  cutgen {json.dumps(r.get('cutgen', {}).get('kernel'))}")
    print(f"== gate against {parent}")
    for v in variants[1:]:
        print(f"  {v} " + gate("cut_partial", cut[parent], cut[v]))
        print(f"  {v} " + gate("ms_per_step", step[parent], step[v]))
    print("== dumped outputs against the parent's first run")
    pd = sorted(glob.glob(os.path.join(d, f"dump_{parent}_*")))[0]
    for v in variants[1:]:
        for dd in sorted(glob.glob(os.path.join(d, f"dump_{v}_*"))):
            res = []
            for name in DUMPS:
                a, b = np.load(os.path.join(pd, name + ".npy")), np.load(os.path.join(dd, name + ".npy"))
                if a.shape == b.shape and a.tobytes() == b.tobytes():
                    res.append(f"{name} byte-equal")
                elif a.shape != b.shape:
                    res.append(f"{name} SHAPES DIFFER {a.shape} {b.shape}")
                else:
                    den = np.maximum(1.0, np.abs(a.astype(np.float64)))
                    res.append(f"{name} differs: max |diff| / max(1, |parent|) {np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / den):.3e}")
            print(f"  {os.path.basename(dd)}: " + ", ".join(res))


if __name__ == "__main__":
    main()
