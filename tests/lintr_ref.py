"""Host restatement (numpy) of the LINTR streams, the reference of
tests/test_lintr_host.py and tests/test_gpu_lintr.py.  Built on tests/vr_ref.py and
tests/blocks_ref.py; shares no code with the library.

A table is (dists, blocks, lintr): `dists` and `blocks` as in blocks_ref with ("LINTR",) for a LINTR
member, `lintr` a list of (members, constants, latents, rows): element indices in the block's
order, one constant per member, the latents as vr_ref distributions, and per member the entries
(block-local latent index, coefficient) of its row of H.  The latents of all blocks are numbered
0 .. Q-1 in block order; latent l is column k + l of vr_ref's stream of an independent layout of
k + Q elements.  All functions return element VALUES, shape (N, k)."""
import functools
import os

import numpy as np

from tests import blocks_ref as B
from tests import vr_ref as V

_PLACEHOLDER = ("UNIFORM", 0.0, 0.0)


def table_of(sto, positions):
    """(dists, blocks, lintr) of a sqlp_amd.smps.spStoType in the layout `positions`."""
    index = {p: e for e, p in enumerate(positions)}
    lmember = {p for b in sto.lintr for p in b.positions}
    member = {p for b in sto.blocks for p in b.positions}
    dists = [("LINTR",) if p in lmember else ("BLOCK",) if p in member else sto.indep[p] for p in positions]
    blocks = [([index[p] for p in b.positions], list(b.probs), np.asarray(b.values, dtype=np.float64).reshape(len(b.probs), -1))
              for b in sto.blocks]
    lintr = [([index[p] for p in b.positions], list(b.constants), list(b.latents), [list(r) for r in b.rows]) for b in sto.lintr]
    return dists, blocks, lintr


def latents(plan, k, lintr, N, seed, first=0):
    """xi (N, Q): columns k .. k+Q-1 of the independent stream of k + Q elements under the plan."""
    lat = [d for L in lintr for d in L[2]]
    ext = [_PLACEHOLDER] * k + lat
    if plan == "iid":
        full = V.iid(ext, N, seed, first)
    elif plan == "antithetic":
        full = V.antithetic(ext, N, seed, first)
    else:
        full = V.lhs(ext, plan[1], N, seed, first)
    return full[:, k:]


def apply(lintr, xi, out):
    """Members into out: v = c_j, then v = v + (h * xi_l) per entry in order.  Elementwise numpy:
    one fp64 rounding per product and per sum, no fma."""
    l0 = 0
    for members, constants, lat, rows in lintr:
        for j, e in enumerate(members):
            v = np.full(xi.shape[0], float(constants[j]))
            for l, h in rows[j]:
                v = v + float(h) * xi[:, l0 + l]
            out[:, e] = v
        l0 += len(lat)
    return out


def draw(plan, dists, blocks, lintr, N, seed, first=0):
    """plan: "iid", "antithetic" or ("lhs", S)."""
    k = len(dists)
    base = [_PLACEHOLDER if d[0] == "LINTR" else d for d in dists]
    out = B.draw(plan, base, blocks, N, seed, first)
    if lintr:
        apply(lintr, latents(plan, k, lintr, N, seed, first), out)
    return out


# ---- lands3t at lands' x_EV: the exact expectation and the restated streams, solved on the CPU ----------
LANDS3T_SEED, LANDS3T_N = 4242, 32768
LANDS3T_PLANS = ["iid", "antithetic", ("lhs", 16)]


def group_of(plan):
    return 1 if plan == "iid" else 2 if plan == "antithetic" else plan[1]


@functools.lru_cache(maxsize=None)
def lands3t():
    """dict: sto, positions, rows, support (6, 3), probs, obj (the six recourse values by the
    oracle's LP), exact (their expectation), x, c1, and per plan (mean, standard error) of the
    recourse over the restated stream (seed 4242, N = 32768; group means for the two plans),
    values (the stream)."""
    from oracle import lp_highs
    from sqlp_amd import smps
    from tests import instances as I
    cor, tim, sto = smps.load_smps(os.path.join(I.DATA, "lands3t"))
    sp2 = smps.get_smps_stage_template(cor, tim, 2)
    positions, rows, cols = smps.scenario_positions(sp2, sto)
    assert (cols < 0).all()
    support, probs = smps.joint_support(sto, positions)
    x = I.x_ev("lands")
    sp = I.load("lands")["osp2"]                       # the same core file
    obj = []
    for v in support:
        b = sp.r - sp.T @ x
        b[rows] += v - sp.r[rows]
        status, o, _, _ = lp_highs.solve_rhs(sp, b)
        assert status == 0, f"lands3t: the LP at {v} is not optimal"
        obj.append(o)
    obj = np.array(obj)
    exact = float(probs @ obj / probs.sum())
    dists, blocks, lintr = table_of(sto, positions)
    streams = {}
    for plan in LANDS3T_PLANS:
        vals = draw(plan, dists, blocks, lintr, LANDS3T_N, LANDS3T_SEED)
        hit = (vals[:, None, :] == support[None, :, :]).all(axis=2)
        assert (hit.sum(axis=1) == 1).all()
        o = obj[hit.argmax(axis=1)]
        G = group_of(plan)
        gm = V.group_means(o, G)
        streams[plan] = dict(values=vals, obj=o, mean=float(gm.mean()), se=float(gm.std(ddof=1) / np.sqrt(gm.size)))
    c1 = smps.get_smps_stage_template(cor, tim, 1).q
    return dict(cor=cor, tim=tim, sto=sto, sp2=sp2, positions=positions, rows=rows, support=support, probs=probs, obj=obj,
                exact=exact, x=x, c1=np.asarray(c1), streams=streams, table=(dists, blocks, lintr))
