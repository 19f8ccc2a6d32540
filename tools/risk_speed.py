#!/usr/bin/env python3
"""Device time of the quantile selection (twosd_cut_quantile) and of the tail re-formation
(twosd_cut_tail) beside their yardstick, twosd_build_cut on the same epigraph in the same run.

Workload: the bench's epigraph (storm, N scenarios drawn on the device, |V| = 4096 LP duals), one cut
at x_EV, then the selection at `level` and the tail cut at eta = VaR.  Timing: the library's own
device events (twosd_risk_last_ms; twosd_last_timings for the cut's two phases), one warm-up then
every one of three repeats kept, and a host clock around the synchronous calls beside them.

--tree PATH imports sqlp_amd from another checkout (its library built in-tree) instead of this
one: on a checkout without the risk entry points only the cut is timed, which is how the parent
commit's twosd_build_cut is measured in the same run as this commit's kernels.

Prints one JSON line.  --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(f, reps=3):
    f()                   # warm-up
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = f()
        out.append(((time.perf_counter() - t) * 1e3, r))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instance", default="storm")
    ap.add_argument("--scenarios", type=int, default=1 << 20)
    ap.add_argument("--vertices", type=int, default=4096)
    ap.add_argument("--level", type=float, default=0.9)
    ap.add_argument("--seed", type=int, default=20250219)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import torch
    torch.cuda.init()
    from sqlp_amd import smps, twosd
    name = args.instance
    cor, tim, sto = smps.load_smps(os.path.join(tree, "data", "smps", name), name)
    sp2 = smps.get_smps_stage_template(cor, tim, 2)
    with open(os.path.join(tree, "tests", "golden", "ev_x.json")) as f:
        x = np.array(json.load(f)[name]["x"])
    ctx = twosd.SDContext(sp2, sto)
    ctx.compute_basis(x, smps.mean_values(sto))
    ctx.set_distributions(sto)
    N = args.scenarios
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, N, args.seed)
    V = twosd.sdDualVertexSet(ctx)
    src = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(src, 1 << 18, args.seed + 1)
    at = 0
    while len(V) < args.vertices and at < (1 << 18):
        _, _, pis, st = twosd.solve_batch(src, x, at, 16384, want_pi=True)
        V.push_batch(pis[st == 0])
        at += 16384
    if len(V) > args.vertices:
        V.truncate(args.vertices)

    def cut():
        twosd.build_sasa_cut(epi, x, V, tie_rel=1e-12)
        t = ctx.timings_us()
        return float(t[2] + t[3]) / 1e3

    runs = timed(cut)
    out = {"instance": name, "scenarios": N, "vertices": len(V), "k": ctx.k, "tree": os.path.relpath(tree, ROOT),
           "has_risk": hasattr(twosd, "cut_tail"),
           "build_cut_host_ms": [r[0] for r in runs], "build_cut_device_ms": [r[1] for r in runs]}
    if out["has_risk"]:
        q = timed(lambda: (twosd.cut_quantile(epi, args.level), float(twosd.risk_last_ms(ctx)[0])))
        var = q[-1][1][0].var
        t = timed(lambda: (twosd.cut_tail(epi, var), float(twosd.risk_last_ms(ctx)[1])))
        tail = t[-1][1][0]
        out.update({"level": args.level, "var": var, "cvar": q[-1][1][0].cvar, "tail_fraction": tail.d,
                    "cut_quantile_host_ms": [r[0] for r in q], "cut_quantile_device_ms": [r[1][1] for r in q],
                    "cut_tail_host_ms": [r[0] for r in t], "cut_tail_device_ms": [r[1][1] for r in t],
                    # what the kernels must stream: eight passes over score + weight; the deltas of the tail's rows
                    "quantile_model_bytes": 8 * N * 16 + N * 16,
                    "tail_model_bytes": int(N * 24 + tail.d * N * 8 * ctx.k)})
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
