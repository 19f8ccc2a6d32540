"""Host restatement (numpy) of the joint discrete streams, the reference of
tests/test_blocks_host.py and tests/test_gpu_blocks.py.  Built on tests/vr_ref.py (its Philox, its
DISCRETE / UNIFORM inversion, its LHS permutations and its NORMAL paths); shares no code with the
library, and picks a block's realisation by the literal sequential walk, not by a search.

A table is (dists, blocks): `dists` as in vr_ref with ("BLOCK",) for a block member, `blocks` a
list of (members, probs, values): element indices in the block's order (members[0] is the lead),
R probabilities, values[R][n].  All functions return element VALUES, shape (N, k)."""
import math

import numpy as np

from tests import vr_ref as V


def table_of(sto, positions):
    """(dists, blocks) of a sqlp_amd.smps.spStoType in the layout `positions`."""
    index = {p: e for e, p in enumerate(positions)}
    member = {p for b in sto.blocks for p in b.positions}
    dists = [("BLOCK",) if p in member else sto.indep[p] for p in positions]
    blocks = [([index[p] for p in b.positions], list(b.probs), np.asarray(b.values, dtype=np.float64).reshape(len(b.probs), -1))
              for b in sto.blocks]
    return dists, blocks


def element_words(k, blocks):
    """The Philox element word of every element: a block's lead for its members, else e."""
    ew = np.arange(k)
    for members, _, _ in blocks:
        ew[np.asarray(members)] = members[0]
    return ew


def walk(probs, u):
    """i = 0, cp = p_0; while (cp <= u && i < R - 1) cp = cp + p_{++i} -- for an array of u."""
    u = np.asarray(u, dtype=np.float64)
    p = np.asarray(probs, dtype=np.float64)
    cp = np.full(u.shape, p[0])
    i = np.zeros(u.shape, dtype=np.int64)
    go = np.ones(u.shape, dtype=bool)
    for j in range(1, len(p)):
        go &= cp <= u                      # the walk stops for good at the first cp > u
        cp = np.where(go, cp + p[j], cp)
        i += go
    return i


def _fill_blocks(out, blocks, u):
    """u (N, k), already gathered at the element words: members e_j take V[walk(u[:, lead])][j]."""
    for members, probs, values in blocks:
        i = walk(probs, u[:, members[0]])
        values = np.asarray(values, dtype=np.float64).reshape(len(probs), len(members))
        for j, e in enumerate(members):
            out[:, e] = values[i, j]


def iid(dists, blocks, N, seed, first=0):
    k = len(dists)
    ew = element_words(k, blocks)
    u1, u2 = V.uniforms(seed, first + np.arange(N, dtype=np.uint64), k)
    u1, u2 = u1[:, ew], u2[:, ew]
    out = np.empty((N, k))
    for e, d in enumerate(dists):
        if d[0] == "NORMAL":
            out[:, e] = d[1] + math.sqrt(d[2]) * V.box_muller(u1[:, e], u2[:, e])
        elif d[0] != "BLOCK":
            out[:, e] = V.invert(d, u1[:, e])
    _fill_blocks(out, blocks, u1)
    return out


def antithetic(dists, blocks, N, seed, first=0):
    assert first % 2 == 0 and N % 2 == 0
    k = len(dists)
    ew = element_words(k, blocks)
    g = np.uint64(first) + np.arange(N, dtype=np.uint64)
    odd = (g & np.uint64(1)).astype(bool)
    u1, u2 = V.uniforms(seed, g & ~np.uint64(1), k)
    u1, u2 = u1[:, ew], u2[:, ew]
    um = np.where(odd[:, None], 1.0 - u1, u1)
    out = np.empty((N, k))
    for e, d in enumerate(dists):
        if d[0] == "NORMAL":
            z = V.box_muller(u1[:, e], u2[:, e])
            out[:, e] = d[1] + math.sqrt(d[2]) * np.where(odd, -z, z)
        elif d[0] != "BLOCK":
            out[:, e] = V.invert(d, um[:, e])
    _fill_blocks(out, blocks, um)
    return out


def lhs(dists, blocks, S, N, seed, first=0):
    """The LHS formula with the lead in place of e: permutation of (LHS block, lead), u1 of (g, lead)."""
    k = len(dists)
    ew = element_words(k, blocks)
    u = V.lhs_uniforms(S, N, k, seed, first)[:, ew]
    out = np.empty((N, k))
    for e, d in enumerate(dists):
        if d[0] == "NORMAL":
            z = np.array([V.ncdfinv(max(float(v), V.U_FLOOR)) for v in u[:, e]])
            out[:, e] = d[1] + math.sqrt(d[2]) * z
        elif d[0] != "BLOCK":
            out[:, e] = V.invert(d, u[:, e])
    _fill_blocks(out, blocks, u)
    return out


def draw(plan, dists, blocks, N, seed, first=0):
    """plan: "iid", "antithetic" or ("lhs", S)."""
    if plan == "iid":
        return iid(dists, blocks, N, seed, first)
    if plan == "antithetic":
        return antithetic(dists, blocks, N, seed, first)
    return lhs(dists, blocks, plan[1], N, seed, first)
