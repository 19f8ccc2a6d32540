#!/usr/bin/env python3
"""Device time of a tail handle beside its yardstick, the pick handle of the same cut on the same
commit: twosd_tail_keep (twosd_tail_last_ms), twosd_reform_cuts on the tail handle and
twosd_reform_cuts on the pick handle (twosd_reform_last_ms: [partial sums, finalize]).

Workload: the bench's epigraph (storm, N = 2^20 scenarios drawn on the device, |V| = 4096 LP duals),
one cut at x_EV, M = 32 replicates, the tail at eta = the cut's VaR at each level (0.8 and 0.95: a
fifth and a twentieth of the scenarios).  The expectation is a partial-sum time near nt / n of the
pick handle's: the tail kernels read the tail's rows of the deltas only.

Protocol: every call once as a warm-up, then `--reps` repetitions with the two handles alternating;
every repetition is kept and the median and the spread (min, max) are reported.  The times are the
library's own device events; nothing here runs without a GPU.

Prints one JSON line per level.  --out appends them to a file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": list(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instance", default="storm")
    ap.add_argument("--scenarios", type=int, default=1 << 20)
    ap.add_argument("--vertices", type=int, default=4096)
    ap.add_argument("--replicates", type=int, default=32)
    ap.add_argument("--levels", type=float, nargs="+", default=[0.8, 0.95])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=20250219)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tail_reform_speed: no GPU (nothing is measured without one)")
    torch.cuda.init()
    from sqlp_amd import smps, twosd
    name = args.instance
    cor, tim, sto = smps.load_smps(os.path.join(ROOT, "data", "smps", name), name)
    sp2 = smps.get_smps_stage_template(cor, tim, 2)
    with open(os.path.join(ROOT, "tests", "golden", "ev_x.json")) as f:
        x = np.array(json.load(f)[name]["x"])
    ctx = twosd.SDContext(sp2, sto)
    ctx.compute_basis(x, smps.mean_values(sto))
    ctx.set_distributions(sto)
    N, M = args.scenarios, args.replicates
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
    cut = twosd.build_sasa_cut(epi, x, V, tie_rel=1e-12, keep_picks=True)
    lines = []
    for level in args.levels:
        eta = twosd.cut_quantile(epi, level).var
        keep = []
        for rep in range(args.reps + 1):               # the first is the warm-up
            h = twosd.keep_tail_of_last_cut(epi, eta)
            if rep:
                keep.append(twosd.tail_last_ms(ctx))
            if rep < args.reps:
                twosd.picks_release(ctx, h)
                epi._pick_handles.discard(h)
        nt = twosd.tail_info(ctx, h).nt
        tail, pick = [], []
        for rep in range(args.reps + 1):
            Rt = twosd.reform_cuts(epi, [h], M, args.seed)
            mt = twosd.reform_last_ms(ctx).copy()
            Rp = twosd.reform_cuts(epi, [cut], M, args.seed)
            mp = twosd.reform_last_ms(ctx).copy()
            if rep:
                tail.append(mt)
                pick.append(mp)
        tail, pick = np.array(tail), np.array(pick)
        out = {"instance": name, "scenarios": N, "vertices": len(V), "k": ctx.k, "replicates": M, "level": level, "eta": eta,
               "nt": nt, "tail_fraction": nt / N, "reps": args.reps,
               "tail_keep_device_ms": summary(keep),
               "reform_tail_partial_ms": summary(tail[:, 0].tolist()), "reform_tail_finalize_ms": summary(tail[:, 1].tolist()),
               "reform_pick_partial_ms": summary(pick[:, 0].tolist()), "reform_pick_finalize_ms": summary(pick[:, 1].tolist()),
               "partial_ratio_tail_over_pick": float(np.median(tail[:, 0]) / np.median(pick[:, 0])),
               # the tail row against the identity row of the pick handle weighed by the flags is the tests' business;
               # here only that both calls gave finite rows of the expected weight
               "tail_weight_share": float(Rt.weight_mark[0, 0] / Rp.weight_mark[0, 0]),
               # what the S kernels must stream per replicate group of 16: the rows of the deltas, 8 k bytes each
               "model_bytes_tail": int(-(-M // 16) * nt * 8 * ctx.k), "model_bytes_pick": int(-(-M // 16) * N * 8 * ctx.k)}
        twosd.picks_release(ctx, h)
        epi._pick_handles.discard(h)
        line = json.dumps(out)
        print(line)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
