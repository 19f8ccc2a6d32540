#!/usr/bin/env python3
"""Speed of the feasibility path on the GPU (profiles/feas/README.md).

  scan   feas_scan_kernel on storm's sampled deltas (default 2^20 scenarios) with J = 1, 16, 64 rays:
         64 dual vertices of storm stand in for rays (storm itself has complete recourse).  Device
         events around the scan and merge kernels (twosd_last_ray_stats), warm-up, repeats; against
         the time to read the N k deltas once at the HBM rate 6.3 TB/s.
  rays   twosd_solve_rays next to twosd_solve_batch on the generated incomplete-recourse template
         (tests/feas_cases.py, m_lp = 130) with 65,536 scenarios of which about a tenth are
         infeasible: host clock around calls that end in a device synchronise; the re-solves the
         scan filter saved.

Usage (repository root, on the GPU): python tools/feas_speed.py [scan|rays|all] [--n N] [--out FILE]
Prints one JSON line per measurement; a missing GPU is an error."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3          # achievable HBM rate of the MI355X (float4 copy)
FP64_VEC_TFLOPS = 78.6  # vector fp64 peak (FMA); the scan's separate multiply and add run at half of it


def med(v):
    return float(np.median(v))


def scan(N, reps, out):
    from sqlp_amd import smps, twosd
    from tests import instances as I
    inst = I.load("storm")
    ctx = twosd.SDContext(inst["sp2"], inst["sto"])
    x = I.x_ev("storm")
    ctx.compute_basis(x, smps.mean_values(inst["sto"]))
    ctx.set_distributions(inst["sto"])
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, N, 20240, first_index=0)
    small = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(small, 8192, 7, first_index=0)
    twosd.solve_push(small, x, 0, 8192)
    V = twosd.sdDualVertexSet(ctx).matrix()
    assert len(V) >= 64, len(V)
    F = twosd.sdFeasRaySet(ctx)
    k = ctx.k
    floor_ms = 1e3 * N * k * 8 / (HBM_TBS * 1e12)
    for J in (1, 16, 64):
        F.clear()
        F.push_batch(V[:J])
        assert F.size == J
        for _ in range(3):
            twosd.feas_scan(epi, x)
        dev, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            sc = twosd.feas_scan(epi, x)
            wall.append(1e3 * (time.perf_counter() - t0))
            dev.append(1e-3 * twosd.last_scan_us(ctx))
        flop_ms = 1e3 * 2.0 * J * k * N / (0.5 * FP64_VEC_TFLOPS * 1e12)
        rec = dict(what="feas_scan_kernel", instance="storm", N=N, k=k, J=J, reps=reps, kernel_ms=med(dev), kernel_ms_min=min(dev),
                   kernel_ms_max=max(dev), call_ms=med(wall), read_floor_ms=floor_ms, fp64_floor_ms=flop_ms,
                   times_read_floor=med(dev) / floor_ms, delta_gbytes=N * k * 8 / 1e9, achieved_tbs=N * k * 8 / (1e9 * med(dev)),
                   n_cut_off=int(sc.n_cut_off))
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
    ctx.close()


def rays(N, reps, out):
    from oracle import cpu
    from sqlp_amd import twosd
    from tests import feas_cases as FC
    S = FC.incomplete_template(130, 3, False, 9, 3.7, "speed")
    vals = FC.values(S, N, seed=2)
    K = S.canon
    lp = cpu.CpuLP(K.W, K.q, K.sense)
    st0, _, head, _ = lp.solve_from_slack(FC.rhs_lp(S, FC.X0, vals[:1])[0])
    assert st0 == 0
    ctx = twosd.SDContext(S.sp2, positions=S.positions)
    ctx.set_basis(head)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals)
    F = twosd.sdFeasRaySet(ctx)
    x = FC.X0
    obj = np.zeros(N)
    st = np.zeros(N, dtype=np.int32)

    def batch():
        import ctypes as C
        from sqlp_amd._lib import ptr
        t0 = time.perf_counter()
        rc = ctx.lib.twosd_solve_batch(ctx.h, epi.index, ptr(np.ascontiguousarray(x)), 0, N, ptr(obj), None, None, ptr(st))
        assert rc in (0, -4), rc           # TWOSD_E_LP: some scenario is infeasible, as intended here
        return 1e3 * (time.perf_counter() - t0)

    def ray_pass(cap):
        F.clear()
        t0 = time.perf_counter()
        rb = twosd.solve_rays(epi, x, 0, N, cap=cap, push=True)
        return 1e3 * (time.perf_counter() - t0), rb

    for _ in range(2):
        batch()
        ray_pass(256)
    tb = [batch() for _ in range(reps)]
    tr, rb = [], None
    for _ in range(reps):
        t, rb = ray_pass(256)
        tr.append(t)
    resolved, filtered = twosd.last_ray_stats(ctx)
    rec = dict(what="twosd_solve_rays vs twosd_solve_batch", template="incomplete m_lp=130 k=3", N=N, reps=reps,
               infeasible=int(rb.n_infeasible), infeasible_share=rb.n_infeasible / N, rays=int(len(rb.scen)), F_size=F.size,
               solve_batch_ms=med(tb), solve_batch_ms_min=min(tb), solve_batch_ms_max=max(tb), solve_rays_ms=med(tr), solve_rays_ms_min=min(tr),
               solve_rays_ms_max=max(tr), resolved=resolved, filtered_by_scan=filtered)
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=["scan", "rays", "all"])
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.devnull, help="append the JSON lines to this file too")
    a = ap.parse_args()
    with open(a.out, "a") as out:
        if a.what in ("scan", "all"):
            scan(a.n or (1 << 20), a.reps, out)
        if a.what in ("rays", "all"):
            rays(a.n or 65536, a.reps, out)


if __name__ == "__main__":
    main()
