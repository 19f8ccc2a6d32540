"""Unrounded twosd_last_refresh_ms phases of the storm refresh (16384 training scenarios, pool 4096, the
bench's sizes), cycling over three x points with a 65536-scenario solve between refreshes (the auto cap's
reference).  One JSON line: per x point and phase the median over the timed refreshes."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from tests import instances as I
from tests.test_gpu_pool_refresh import _sd_x
from sqlp_amd import smps, twosd
inst = I.load("storm")
x_ev = I.x_ev("storm")
x2 = _sd_x(3)
xs = [x_ev, x2, x_ev + 0.6 * (x2 - x_ev)]
ctx = twosd.SDContext(inst["sp2"], inst["sto"])
ctx.compute_basis(x_ev, smps.mean_values(inst["sto"]))
ctx.set_distributions(inst["sto"])
tr = twosd.sdEpigraph(ctx, 1.0, 0.0)
twosd.add_sampled_scenarios(tr, 16384, 4242)
ev = twosd.sdEpigraph(ctx, 1.0, 0.0)
twosd.add_sampled_scenarios(ev, 65536, 99)
rec = {i: [] for i in range(len(xs))}
sizes = []
for cyc in range(13):
    for i, x in enumerate(xs):
        P = ctx.pool_refresh(tr, x, 0, 16384, 4096)
        ms = list(ctx.last_refresh_ms())
        twosd.solve_batch(ev, x, 0, 65536, want_pi=False)
        if cyc >= 3:
            rec[i].append(ms)
            sizes.append(P)
out = {"lib": os.environ.get("TWOSD_LIB", "new"), "pool": sorted(set(sizes)), "piv": ctx.lp_stats()[0]}
for i in rec:
    a = np.array(rec[i])
    out[f"x{i}"] = [float(v) for v in np.median(a, axis=0)]
print(json.dumps(out))
