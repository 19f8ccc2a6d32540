#!/usr/bin/env python3
"""Speed of the bootstrap re-formation (twosd_reform_cuts) against its yardstick, twosd_build_cut
on the same epigraph in the same run.

Workload: the bench's epigraph (storm, N scenarios drawn on the device, |V| = 4096 LP duals), H
cuts built at slightly different x with their picks kept, M bootstrap replicates.  Timing: a host
clock around the synchronous calls (each ends in a device synchronise), one warm-up then best of
three, and the library's own device events for the re-formation's two phases
(twosd_reform_last_ms).  The byte model is what one pass per handle must stream:
H N (8 k + 12) -- the deltas, the weight and the pick of every scenario, once per handle (the
kernel re-reads the deltas once per group of 16 replicates; the groups of a chunk are adjacent
blocks, so the re-reads are meant to hit L2 / the Infinity Cache).

--sampling lists sampling plans (antithetic, lhsS) whose grouped re-formation (reform_cuts with
sampling=: whole groups resampled) is timed on the same epigraph and handles beside the i.i.d. call,
the same way (warm-up, best of three, every repeat kept); the scenario count must be whole groups of
each.  The epigraph's own stream stays the i.i.d. one: the work does not depend on the values.

--tree PATH imports sqlp_amd from another checkout (its library built in-tree) instead of this one,
as tools/risk_speed.py does: the parent commit's re-formation is then measured in the same job.
reform_device_ms_runs keeps the two phases' device times of every repeat.

Prints one JSON line.  --out also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK_GBS = 8000.0     # MI355X HBM3E peak


def runs_of(f, reps=3):
    f()                   # warm-up
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def best_of(f, reps=3):
    return min(runs_of(f, reps))


def plan_of(name):
    from sqlp_amd import twosd
    if name == "iid":
        return None
    if name == "antithetic":
        return twosd.Sampling.antithetic()
    if name.startswith("lhs") and name[3:].isdigit():
        return twosd.Sampling.lhs(int(name[3:]))
    raise SystemExit(f"--sampling: unknown plan {name!r} (iid, antithetic, lhsS)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instance", default="storm")
    ap.add_argument("--scenarios", type=int, default=1_000_000)
    ap.add_argument("--vertices", type=int, default=4096)
    ap.add_argument("--handles", type=int, default=20)
    ap.add_argument("--replicates", type=int, default=32)
    ap.add_argument("--seed", type=int, default=20250219)
    ap.add_argument("--sampling", default="", help="comma-separated plans to time beside the i.i.d. call: antithetic, lhs64, ...")
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
    N, H, M = args.scenarios, args.handles, args.replicates
    plans = {p: plan_of(p) for p in args.sampling.split(",") if p}
    for p, plan in plans.items():
        if plan is not None and N % plan.group:
            raise SystemExit(f"--sampling {p}: {N} scenarios are no whole number of groups of {plan.group}")
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
    cuts = [twosd.build_sasa_cut(epi, x * (1.0 + 0.002 * j), V, tie_rel=1e-12, keep_picks=True) for j in range(H)]
    cut_ms = best_of(lambda: twosd.build_sasa_cut(epi, x, V, tie_rel=1e-12))
    cut_kernel_ms = float(ctx.timings_us()[2] + ctx.timings_us()[3]) / 1e3
    one_ms = best_of(lambda: twosd.reform_cuts(epi, cuts[:1], M, args.seed))
    dev_runs = []

    def all_handles():
        twosd.reform_cuts(epi, cuts, M, args.seed)
        dev_runs.append([float(v) for v in twosd.reform_last_ms(ctx)])
    all_runs = runs_of(all_handles)
    dev_runs = dev_runs[1:]     # without the warm-up
    all_ms = min(all_runs)
    id_ms = best_of(lambda: twosd.reform_cuts(epi, cuts, 0, args.seed))
    R = twosd.reform_cuts(epi, cuts, M, args.seed)
    dev_ms = [float(v) for v in twosd.reform_last_ms(ctx)]
    err = max(abs(R.alpha[0, j] - c.alpha) / (1 + abs(c.alpha)) for j, c in enumerate(cuts))
    grouped = {}
    for p, plan in plans.items():
        runs = runs_of(lambda: twosd.reform_cuts(epi, cuts, M, args.seed, sampling=plan))
        grouped[p] = {"reform_ms": min(runs), "reform_ms_runs": runs, "reform_device_ms": [float(v) for v in twosd.reform_last_ms(ctx)],
                      "over_iid": min(runs) / all_ms}
    k = ctx.k
    model = H * N * (8 * k + 12)
    out = {"instance": name, "tree": os.path.relpath(tree, ROOT), "scenarios": N, "vertices": len(V), "k": k, "handles": H, "replicates": M,
           "build_cut_ms": cut_ms, "build_cut_kernels_ms": cut_kernel_ms,
           "reform_ms": all_ms, "reform_ms_runs": all_runs, "reform_device_ms": dev_ms, "reform_device_ms_runs": dev_runs, "reform_ms_per_handle": all_ms / H, "reform_one_handle_ms": one_ms,
           "reform_identity_only_ms": id_ms,
           "model_bytes": model, "achieved_GBs": model / (all_ms * 1e-3) / 1e9,
           "fraction_of_hbm_peak": model / (all_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
           "handle_over_cut": (all_ms / H) / cut_ms, "identity_row_max_rel_err": err}
    if grouped:
        out["sampling"] = grouped
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
