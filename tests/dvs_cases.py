"""Directed inputs for the device dual vertex set (sqlp_amd/csrc/dvs_kernel.hip, dvs_keys.h) and a
NumPy restatement of its key, shared by tests/test_dvs_cases.py (the conditions on the inputs,
proved with the oracle alone) and tests/test_gpu_dvs.py (the exact GPU comparisons).  A plain
helper module like tests/synth_cases.py: no GPU, no test functions.

The key of a vector, as dvs_keys.h and dvs_key_kernel define it:
  hash  = bits of round16(sum_i |v_i|), added in index order               (twosd_ref.hash_dual_rows)
  fp    = mix64((sum_i mix64(comp_bits(v_i) ^ (0xD6E8FEB86659FD93 (i + 1)))) ^ hash)   mod 2^64
  nan   = any component is NaN
and the digest of a set (twosd_dvs_fingerprint): size 0x9E3779B97F4A7C15 + sum_i fp_i (2 i + 1)
mod 2^64.  round16 and the hash are the oracle's (oracle/twosd_ref.py), not restated here."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from oracle import twosd_ref as R

U64 = np.uint64
GOLDEN = 0x9E3779B97F4A7C15
POS_MULT = 0xD6E8FEB86659FD93
MASK64 = (1 << 64) - 1


def bits(a) -> np.ndarray:
    """The uint64 view of a float64 array: the comparison that sees -0.0 and NaN."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def mix64(z) -> np.ndarray:
    """dvs_keys.h mix64 (the splitmix64 finaliser) on uint64 arrays, mod 2^64."""
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64))
    with np.errstate(over="ignore"):
        z = z + U64(GOLDEN)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def comp_bits(P) -> np.ndarray:
    """dvs_keys.h comp_bits: the bits of round16 with -0.0 folded onto +0.0."""
    r = R.round16_vec(P)
    return bits(np.where(r == 0.0, 0.0, r))


def key(P):
    """(hash, fp, has_nan) of every row of P, as dvs_key_kernel computes them."""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    h = R.hash_dual_rows(P)
    with np.errstate(over="ignore"):
        pos = U64(POS_MULT) * np.arange(1, P.shape[1] + 1, dtype=np.uint64)
    f = mix64(comp_bits(P) ^ pos[None, :]).reshape(P.shape).sum(axis=1, dtype=np.uint64)
    return h, mix64(f ^ h), np.isnan(P).any(axis=1)


def digest(fps) -> int:
    """twosd_dvs_fingerprint of a set whose vertices have the fingerprints fps, in set order."""
    acc = len(fps) * GOLDEN
    for i, f in enumerate(np.asarray(fps, dtype=np.uint64).tolist()):
        acc += f * (2 * i + 1)
    return acc & MASK64


def set_digest(V) -> int:
    """The digest of the set whose rows are V (a matrix, in set order)."""
    V = np.asarray(V, dtype=np.float64)
    return digest(key(V)[1] if len(V) else [])


# ---- edge_rows ----------------------------------------------------------------------------------
DBL_MAX = np.finfo(np.float64).max
# name -> value.  round16 keeps 16 significant bits: for 2^e <= |x| < 2^(e+1) it rounds to a
# multiple of 2^(e-15), half to even, by scaling with 2^digits, digits = 15 - e.
EDGE_VALUES = {
    "+0": 0.0, "-0": -0.0,
    "+min": 5e-324, "-min": -5e-324,
    # digits = 1024: the scale 2^digits overflows and round16 keeps x (all of |x| < 2^-1008)
    "2^-1009": 2.0 ** -1009, "2^-1009(1+2^-20)": 2.0 ** -1009 * (1 + 2.0 ** -20),
    # digits = 1023: 2^1023 is the largest finite scale, so from 2^-1008 on x is rounded
    "2^-1008": 2.0 ** -1008, "2^-1008(1+2^-20)": 2.0 ** -1008 * (1 + 2.0 ** -20),
    "2^-1007(1+2^-17)": 2.0 ** -1007 * (1 + 2.0 ** -17), "2^-1007(1+2^-18)": 2.0 ** -1007 * (1 + 2.0 ** -18),
    "1": 1.0, "1+2^-16": 1 + 2.0 ** -16, "1+3*2^-16": 1 + 3 * 2.0 ** -16, "1+2^-14": 1 + 2.0 ** -14,
    "2-2^-17": 2 - 2.0 ** -17, "2": 2.0,
    # digits = -2 (the digits < 0 branch): multiples of 4
    "2^17": 2.0 ** 17, "2^17+0.5": 2.0 ** 17 + 0.5, "2^17+1": 2.0 ** 17 + 1, "2^17+2": 2.0 ** 17 + 2,
    "2^17+3": 2.0 ** 17 + 3, "2^17+4": 2.0 ** 17 + 4, "2^17+6": 2.0 ** 17 + 6, "2^17+8": 2.0 ** 17 + 8,
    "1.7e308": 1.7e308, "+max": DBL_MAX, "-max": -DBL_MAX,     # round16(DBL_MAX) overflows: kept
    "+inf": np.inf, "-inf": -np.inf, "nan": np.nan,
}
# pairs whose components are equal after round16 (ties go to even; 2 - 2^-17 carries into the next
# binade) and pairs that stay apart
EDGE_EQUAL = [("+0", "-0"), ("2^-1008", "2^-1008(1+2^-20)"), ("2^-1007(1+2^-17)", "2^-1007(1+2^-18)"), ("1+2^-16", "1"),
              ("1+3*2^-16", "1+2^-14"), ("2-2^-17", "2"), ("2^17+0.5", "2^17"), ("2^17+1", "2^17"), ("2^17+2", "2^17"),
              ("2^17+3", "2^17+4"), ("2^17+6", "2^17+8")]
EDGE_APART = [("2^-1009", "2^-1009(1+2^-20)"), ("+min", "-min"), ("+min", "+0"), ("1", "1+2^-14"), ("2^17", "2^17+4"),
              ("1.7e308", "+max"), ("+max", "-max"), ("+max", "+inf"), ("+inf", "-inf"), ("nan", "+inf")]
EDGE_DOUBLES = [("-0", "+0"), ("+inf", "-inf"), ("+max", "+max"), ("nan", "+inf"), ("1+2^-16", "2^17+3"), ("+min", "-max"),
                ("2^-1009", "2-2^-17")]


def edge_positions(m):
    return sorted({p for p in (0, 63, 64, m - 1) if 0 <= p < m})


def edge_rows(m, seed=1):
    """Copies of one base vector with one or two components replaced by edge values, at the
    positions 0, 63, 64 and m - 1 (lane 0, the last lane, the second round of the key kernel's
    lane loop, the last component).  rows: the vectors in push order; index[(position, name)]:
    the row with that one replacement; splits: batch split points for a push in several batches.
    With m >= 2 also: rows whose L1 sum overflows to inf (two apart, one equal), [inf, 1, ...]
    against [inf, 2, ...] and [-inf, 1, ...], and a -0.0 row ahead of its 0.0 twin (the single
    replacements push 0.0 first).  The last rows repeat earlier ones."""
    rng = np.random.default_rng(1000 * seed + m)
    base = np.round(rng.normal(size=m) * 10.0, 4)
    base[base == 0.0] = 1.5
    rows, index = [], {}
    pos = edge_positions(m)
    for p in pos:
        for name, val in EDGE_VALUES.items():
            v = base.copy()
            v[p] = val
            index[(p, name)] = len(rows)
            rows.append(v)
    if m >= 2:
        p, q = pos[0], pos[-1]
        for a, b in EDGE_DOUBLES:
            v = base.copy()
            v[p], v[q] = EDGE_VALUES[a], EDGE_VALUES[b]
            rows.append(v)
        big = base.copy()
        big[0] = big[1] = 1.7e308
        for f in (1.0, 1 - 2.0 ** -10, 1 - 2.0 ** -30):      # apart from the first / equal to it
            v = big.copy()
            v[1] *= f
            index[("overflow", f)] = len(rows)
            rows.append(v)
        for a, b in ((np.inf, 1.0), (np.inf, 2.0), (-np.inf, 1.0)):
            v = base.copy()
            v[0], v[1] = a, b
            index[("inf", a, b)] = len(rows)
            rows.append(v)
        for z in (-0.0, 0.0):
            v = 2.0 * base
            v[q] = z
            index[("twin", "-0" if np.signbit(z) else "+0")] = len(rows)
            rows.append(v)
    first = len(rows)
    rows += [rows[i].copy() for i in rng.integers(0, first, size=24)]
    rows = np.array(rows)
    splits = [s for s in (1, 2, 17, 64, 65, first) if s < len(rows)]
    return SimpleNamespace(m=m, rows=rows, index=index, positions=pos, splits=splits, n_first=first)


# ---- hash_split_pairs -----------------------------------------------------------------------------
def _pair_stream(m, rng, n):
    """Vectors whose components all survive a factor 1 + 2^-18 under round16 except up to three
    free ones: the others are k / 8 with |k| <= 1024 (11 significant bits, so the factor moves
    them by less than half a unit of the 16th bit); the free ones are np.round(normal * {1, 10,
    1000}, 4).  The sum of such a row still has more than 16 significant bits."""
    k = rng.integers(1, 1025, size=(n, m)) * rng.choice([-1.0, 1.0], size=(n, m))
    P = k / 8.0
    for _ in range(min(m, 3)):
        j = rng.integers(0, m, size=n)
        P[np.arange(n), j] = np.round(rng.normal(size=n) * rng.choice([1.0, 10.0, 1000.0], size=n), 4)
    return P


def hash_split_pairs(m, n=8, seed=5):
    """split: n pairs (v, v (1 + 2^-18)) with every component round16-equal and different hashes:
    two vertices for the reference (dual_set.jl:29).  mirror: n pairs with equal hashes and one
    component apart.  Both (n, 2, m), searched from a seeded stream; m >= 2."""
    assert m >= 2
    rng = np.random.default_rng(1000 * seed + m)
    split, mirror = [], []
    for _ in range(50):
        P = _pair_stream(m, rng, 4000)
        Q = P * (1 + 2.0 ** -18)
        ok = (bits(R.round16_vec(P)) == bits(R.round16_vec(Q))).all(axis=1) & (R.hash_dual_rows(P) != R.hash_dual_rows(Q))
        split += [np.stack([P[i], Q[i]]) for i in np.flatnonzero(ok)[: n - len(split)]]
        P = _pair_stream(m, rng, 4000)                       # other vectors for the mirror pairs
        M = P.copy()
        j = np.abs(P).argmin(axis=1)
        M[np.arange(len(P)), j] *= 1 + 2.0 ** -12
        ok = (R.round16_vec(P) != R.round16_vec(M)).any(axis=1) & (R.hash_dual_rows(P) == R.hash_dual_rows(M))
        mirror += [np.stack([P[i], M[i]]) for i in np.flatnonzero(ok)[: n - len(mirror)]]
        if len(split) == n and len(mirror) == n:
            break
    assert len(split) == n and len(mirror) == n, (m, len(split), len(mirror))
    return SimpleNamespace(m=m, split=np.array(split), mirror=np.array(mirror))


def pair_rows(H):
    """The pairs as one batch: split pairs, mirror pairs, then every first member once more."""
    m = H.m
    return np.vstack([H.split.reshape(-1, m), H.mirror.reshape(-1, m), H.split[:, 0], H.mirror[:, 0]])


# ---- wrap_rows ------------------------------------------------------------------------------------
TCAP0 = 1024      # the set's first table (ensure_capacity) and the batch table for count <= 512


def stream_rows(m, n, seed):
    return np.round(np.random.default_rng(1000 * seed + m).normal(size=(n, m)), 4)


def wrap_rows(m, tcap=TCAP0, n_stream=20000, seed=1):
    """The vectors of a seeded stream whose home slot fp & (tcap - 1) is one of the last two of a
    table of tcap slots.  Pushed into a set of fewer than tcap / 2 vertices they crowd onto those
    two slots, so all but two of them probe past the last slot back to slot 0, in the set's table
    and (as one batch) in the batch table."""
    P = stream_rows(m, n_stream, seed)
    home = key(P)[1] & U64(tcap - 1)
    return P[home >= U64(tcap - 2)]


def filler_rows(m, n, seed=2):
    """n vectors that share no key with wrap_rows (ten times its scale)."""
    return 10.0 * stream_rows(m, n, seed) + 100.0


WRAP_AGAIN = 50


def wrap_filler(m, W):
    """The vertices pushed ahead of the wrap rows W so that the pushes filler, W, [W, WRAP_AGAIN
    filler rows] end at size + count == tcap / 2 exactly: the fullest the first table gets."""
    return filler_rows(m, TCAP0 // 2 - 2 * len(W) - WRAP_AGAIN)


# ---- contention_batch -------------------------------------------------------------------------------
MAX_WAVES = 4 * 8192          # nblocks_for: at most 8192 blocks of four wavefronts, one candidate each per round


def contention_batch(m, n=40000, nbase=37, nlate=7, seed=9):
    """n rows drawn from nbase base vectors; about a quarter are the base times 1 + 2^-40 (the same
    key, other bits, so the kept representative shows which row won); about 0.5 % have a NaN and
    are appended each; the last nlate base vectors first occur after row MAX_WAVES + 232, in the
    second round of the grid-stride loops."""
    rng = np.random.default_rng(1000 * seed + m)
    base = np.round(rng.normal(size=(nbase, m)) * 10.0, 4) + np.arange(nbase)[:, None]
    late_from = MAX_WAVES + 232
    pick = rng.integers(0, nbase - nlate, size=n)
    pick[late_from:] = rng.integers(0, nbase, size=n - late_from)
    rows = base[pick]
    rows[rng.random(n) < 0.25] *= 1 + 2.0 ** -40
    nan = np.flatnonzero(rng.random(n) < 0.005)
    rows[nan, rng.integers(0, m, size=len(nan))] = np.nan
    return SimpleNamespace(m=m, rows=rows, base=base, pick=pick, nan=nan, nbase=nbase, nlate=nlate, late_from=late_from)


# ---- growth_script ----------------------------------------------------------------------------------
# The host logic the script walks through, dvs_kernel.hip:
#   ensure_capacity, need = size + count:
#     :233-234  V, hash, fp regrow at need > cap to max(need, 2 cap + 256); cap starts at 0: 256, 768, 1792, 3840
#     :242-249  the table regrows at tcap < 2 need to the power of two >= max(1024, 2 need), and is rebuilt
#   dvs_push_device:
#     :264-265  the per-candidate workspace re-allocates at count > its capacity, to max(count, 1024)
#     :273-275  the batch table is the power of two >= max(1024, 2 count), never shrunk
#     :211      nblocks_for: the grid-stride kernels run at most 8192 blocks of four wavefronts (MAX_WAVES above)
#   twosd_dvs_truncate (:371-380) rebuilds the table at its current size
def host_trace(counts_and_truncs):
    """What the host does for a sequence of ("push", count) / ("truncate", size) on sets whose
    sizes are given: per push (need, cap_grew, table_grew, ws_grew, tt_grew, capacities after)."""
    cap = tcap = ws = tt = 0
    out = []
    for op, count, size in counts_and_truncs:
        if op != "push" or count == 0:
            continue
        need = size + count
        e = SimpleNamespace(count=count, size=size, need=need, ws_grew=count > ws, cap_grew=need > cap)
        if e.ws_grew:
            ws = max(count, 1024)
        ttneed = 1024
        while ttneed < 2 * count:
            ttneed <<= 1
        e.tt_grew = ttneed > tt
        tt = max(tt, ttneed)
        if e.cap_grew:
            cap = max(need, 2 * cap + 256)
        e.table_grew = tcap < 2 * need
        if e.table_grew:
            tcap = 1024
            while tcap < 2 * need:
                tcap <<= 1
        e.cap, e.tcap, e.ws, e.tt = cap, tcap, ws, tt
        out.append(e)
    return out


def growth_script(m, seed=3):
    """Steps (op = "push" with rows, "truncate" with size, or "clear"), each with size_after, the
    number of vertices the set must then hold, and a note.  Every push of more than one row mixes
    new vectors with copies of vertices already in the set and of rows of the same batch, a quarter
    of them times 1 + 2^-40 (the same key); some batches hold NaN rows, which always append."""
    rng = np.random.default_rng(1000 * seed + m)
    npool, nnan = 3000, 40
    pool = np.round(rng.normal(size=(npool + nnan, m)) * rng.choice([1.0, 10.0, 1000.0], size=(npool + nnan, 1)), 4)
    pool[np.arange(npool, npool + nnan), rng.integers(0, m, size=nnan)] = np.nan
    members = []                  # pool ids of the set's vertices, in set order
    fresh = [0, npool]            # next unused id: plain, NaN
    steps = []

    def emit(ids, note):
        ids = np.asarray(ids, dtype=np.int64)
        rows = pool[ids].copy()
        rows[rng.random(len(ids)) < 0.25] *= 1 + 2.0 ** -40
        have = set(members)
        for i in ids.tolist():
            if i >= npool or i not in have:
                members.append(i)
                have.add(i)
        steps.append(SimpleNamespace(op="push", rows=rows, size_after=len(members), note=note))

    def push(count, n_new, n_nan=0, note=""):
        new = list(range(fresh[0], fresh[0] + n_new)) + list(range(fresh[1], fresh[1] + n_nan))
        fresh[0] += n_new
        fresh[1] += n_nan
        old = [i for i in members if i < npool]
        n_dup = count - len(new)
        n_old = (n_dup + 1) // 2 if old else 0          # copies of old vertices, then of anything so far
        dup = (rng.choice(old, size=n_old).tolist() if n_old else []) + rng.choice(old + new[:n_new], size=n_dup - n_old).tolist()
        ids = np.array(new + dup, dtype=np.int64)
        emit(rng.permutation(ids), note)

    def truncate(size, note, op="truncate"):
        removed = members[size:]
        del members[size:]
        steps.append(SimpleNamespace(op=op, size=size, size_after=size, note=note))
        kept = [i for i in members if i < npool]
        again = removed + (rng.choice(kept, size=min(len(kept), 40)).tolist() if kept else [])
        emit(rng.permutation(np.array(again, dtype=np.int64)), "re-push of the removed rows and of some kept ones")

    push(1, 1, note="batch of 1; cap 0 -> 256, table 1024, workspace 1024, batch table 1024")
    push(255, 200, n_nan=2, note="need 256 == cap: V stays")
    push(54, 53, note="need 257 > cap: V 256 -> 768")
    push(256, 255, note="need 512: 2 need == tcap, the table stays at 1024; 511 vertices")
    push(2, 1, note="need 513: table 1024 -> 2048, rebuilt from 511 vertices; the copy of an old one must be found; 512")
    push(2, 1, note="513 vertices")
    push(255, 100, n_nan=1, note="need 768 == cap: V stays")
    push(1024, 300, note="batch of 1024 == workspace; need 1638: V 768 -> 1792 and table 2048 -> 4096 in one call; batch table 2048")
    push(1025, 200, n_nan=3, note="batch of 1025 > workspace; batch table 4096; need 1939: V 1792 -> 3840")
    truncate(600, "truncate above 512")
    push(2049, 500, n_nan=5, note="batch of 2049 > workspace; batch table 8192; need 3166: table 4096 -> 8192")
    truncate(300, "truncate below 512 (the table keeps its 8192 slots)")
    truncate(1, "truncate to 1")
    truncate(0, "truncate to 0")
    truncate(0, "clear", op="clear")
    return steps
