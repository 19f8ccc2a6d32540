#!/usr/bin/env python3
"""SHA-256 digests over the raw bytes of every output of the cuts re-formed from stored picks: the
bootstrap re-formation (reform_cuts; reform_partial + reform_finalize) and the tail cut (cut_tail).
Two checkouts whose lines agree in every digest compute the same bits on these inputs.

Inputs:
  lands (k = 3), 2500 scenarios with random weights, three cuts kept at 800, 1600 and 2500
    scenarios (2500: 40 tiles in 10 shards, more shards than the bootstrap's 8 summing segments)
  the generated k = 70 template of tests/test_gpu_risk_tail.py (two elements per lane, general
    bounds: c0 != 0), 300 scenarios, one cut kept
each re-formed with M in {1, 33} replicates i.i.d. (G = 1), in antithetic pairs (G = 2) and in LHS
groups of 64 (a tile inside one group) -- the three instantiations of the streaming kernel.  Every
count must be whole groups, so under G = 64 lands holds 2496 scenarios with cuts kept at 832, 1600
and 2496 (39 tiles, 10 shards) and the template 256.  The tail cut is taken of the last cut of the
i.i.d. epigraphs (2500 and 300 scenarios) at eta below every score, at the 0.7 point of the scores
and above every score.  Every epigraph (each G) is then re-formed once more with pick handles and
tail handles mixed -- [first cut, tail, last cut, tail, tail, tail], the tails cut_tail(keep=True) of
the last cut at the scores' midrange, above every score (the empty list), at their 0.7 point and
below every score (the full list: on lands more shards than summing segments); the four lengths
stand in the case's name -- through the boot kernels' list instantiations.

--tree PATH imports sqlp_amd and tests from another checkout (its library built in-tree).
Prints one JSON line.  --out also writes it to a file."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240229


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import torch
    torch.cuda.init()
    from sqlp_amd import smps, twosd
    from tests import instances as I
    from tests import synth_cases as SC
    from tests.test_gpu_risk_tail import _k70_template

    def context(name):
        if name == "lands":
            inst = I.load("lands")
            ctx = twosd.SDContext(inst["sp2"], inst["sto"])
            x = I.x_ev("lands")
            ctx.compute_basis(x, smps.mean_values(inst["sto"]))
            return ctx, x, I.sample("lands", 2500, 3)
        sp2, positions, vals = _k70_template()
        ctx = twosd.SDContext(sp2, positions=positions)
        ctx.compute_basis(SC.X[0], vals[0])
        return ctx, SC.X[0], vals

    def plan(G):
        return None if G == 1 else twosd.Sampling.antithetic() if G == 2 else twosd.Sampling.lhs(G)

    out = {}
    for name, stages_by_g in (("lands", {1: [800, 1600, 2500], 2: [800, 1600, 2500], 64: [832, 1600, 2496]}),
                              ("k70", {1: [300], 2: [300], 64: [256]})):
        ctx, x, vals = context(name)
        w = np.random.default_rng(21).uniform(0.5, 1.5, size=len(vals))
        for G, stages in stages_by_g.items():
            V = twosd.sdDualVertexSet(ctx)
            epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
            handles, lo = [], 0
            for j, hi in enumerate(stages):
                twosd.add_scenarios(epi, vals[lo:hi], w[lo:hi])
                xs = x * (1.0 + 0.03 * j)
                twosd.solve_push(epi, xs, lo, hi - lo)
                _, mv, _ = twosd._build_cut(epi, xs, 0.0, want_argmax=True)
                handles.append(twosd.keep_picks_of_last_cut(epi))
                lo = hi
            if G == 1:
                srt = np.sort(mv)
                for what, eta in (("below", float(srt[0]) - 1.0), ("p70", float(srt[(7 * len(srt)) // 10])), ("above", float(srt[-1]) + 1.0)):
                    t = twosd.cut_tail(epi, eta)
                    out[f"{name} N={stages[-1]} cut_tail {what}"] = digest([t.alpha], t.beta, [t.tail_weight], [t.total_weight])
            total = epi.total_scenario_weight

            def both(key, hs, M):
                R = twosd.reform_cuts(epi, hs, M, SEED, sampling=plan(G))
                out[key + " reform_cuts"] = digest(R.alpha, R.beta, R.weight_mark, R.total_weight)
                nu, nf = twosd.reform_partial_len(ctx, hs, M)
                u = torch.zeros(nu, dtype=torch.int64, device="cuda")
                f = torch.zeros(nf, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                twosd.reform_partial(epi, hs, M, SEED, 0, total, u.data_ptr(), f.data_ptr(), sampling=plan(G))
                R = twosd.reform_finalize(ctx, hs, M, total, u.data_ptr(), f.data_ptr())
                out[key + " partial+finalize"] = digest(R.alpha, R.beta, R.weight_mark, R.total_weight)

            for M in (1, 33):
                both(f"{name} N={stages[-1]} G={G} M={M}", handles, M)
            # tail handles of the last cut: the full tail, the scores' midrange, their 0.7 point, the empty tail
            srt = np.sort(mv)
            etas = (float(srt[0]) - 1.0, 0.5 * float(srt[0] + srt[-1]), float(srt[(7 * len(srt)) // 10]), float(srt[-1]) + 1.0)
            tails = [twosd.cut_tail(epi, eta, keep=True).picks for eta in etas]
            nts = "/".join(str(twosd.tail_info(ctx, t).nt) for t in tails)
            mixed = [handles[0], tails[1], handles[-1], tails[3], tails[2], tails[0]]
            for M in (1, 33):
                both(f"{name} N={stages[-1]} G={G} M={M} mixed, tails nt={nts}", mixed, M)
            for h in handles + tails:
                twosd.picks_release(ctx, h)
        ctx.close()
    line = json.dumps({"tree": os.path.relpath(tree, ROOT), "digests": out}, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
