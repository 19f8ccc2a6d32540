#!/usr/bin/env python3
"""Relative gaps of the SD loop on lands3b (seeds 11 / 12 / 13, 60 iterations from x_EV, one scenario
per iteration): the incumbent's true objective, enumerated over the six realisations with HiGHS,
against the extensive optimum.  The setup and the references are those of
tests/test_gpu_risk_loop.py, loaded from this checkout.

  tools/risk_loop_gaps.py                the mean-CVaR loop (level 0.8, lam 0.5): lines "RISK seed ..."
  tools/risk_loop_gaps.py --neutral      the risk-neutral master.sd_run: lines "G0 seed ..." and the worst
  --tree PATH                            import sqlp_amd (and oracle, tests) from another checkout with its
                                         library built in-tree -- the parent commit's, for the yardstick g0
"""
import argparse
import importlib.util
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--neutral", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    spec = importlib.util.spec_from_file_location("risk_loop_helpers", os.path.join(ROOT, "tests", "test_gpu_risk_loop.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    L = H.lands3b()
    if not args.neutral:
        for seed in H.SEEDS:
            ctx, cell, _ = H.run_risk(seed)
            true, opt, gap = H.relative_gap(cell.x_incumbent, H.LAM)
            print(f"RISK seed {seed}: objective at the incumbent {true:.9f}, extensive mean-CVaR optimum {opt:.9f}, "
                  f"relative gap {gap:.6e}, eta {cell.eta_incumbent:.6f}, x {cell.x_incumbent.tolist()}")
            ctx.close()
        return
    from sqlp_amd import master, smps, twosd
    gaps = []
    for seed in H.SEEDS:
        ctx = twosd.SDContext(L.sp2, L.sto)
        ctx.compute_basis(L.x_ev, smps.mean_values(L.sto))
        cell = master.sdCell(L.sp1, ctx)
        cell.bind_epigraph(twosd.sdEpigraph(ctx, 1.0, 0.0))
        cell.x_candidate, cell.x_incumbent = L.x_ev.copy(), L.x_ev.copy()
        d = H.draws(seed, H.ITERS)
        it, _ = master.sd_run(cell, lambda i: [L.support[d[i]][None, :]], H.ITERS, min_iter=10 ** 9,
                              stop=lambda c: SimpleNamespace(passed=False))
        true, opt, gap = H.relative_gap(cell.x_incumbent, 0.0)
        print(f"G0 seed {seed}: iterations {it}, objective at the incumbent {true:.9f}, extensive optimum {opt:.9f}, relative gap {gap:.6e}")
        gaps.append(gap)
        ctx.close()
    print(f"G0 worst relative gap = {max(gaps)!r}")


if __name__ == "__main__":
    main()
