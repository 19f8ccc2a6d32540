"""The conditions on the inputs of tests/test_gpu_dvs.py, proved with the oracle alone (no GPU):
every builder of tests/dvs_cases.py gives what it claims (the ties are ties, the pairs split on
the hash or on one component, the wrap rows sit on the last two slots, the contention batch has
exactly the expected vertices, the growth script lands on every threshold of the host code from
both sides), and on the edge inputs the vectorised oracle push_batch that the GPU tests compare
with equals the line-by-line push.  Asserted directly, so that a changed seed cannot silently
hollow out a GPU case."""
import numpy as np
import pytest

from oracle import twosd_ref as R
from tests import dvs_cases as DC

EDGE_MS = [1, 20, 64, 65, 129, 257, 1024]      # templates a, c, d, e, g, i, p of tests/synth_cases.py
PAIR_MS = [3, 20, 65]
WRAP_MS = [20, 65]
CONTENTION_MS = [3, 20]
GROWTH_MS = [65, 257]


def _same_sets(a, b):
    assert len(a) == len(b) and a.hashes == b.hashes
    assert np.array_equal(DC.bits(a.matrix()), DC.bits(b.matrix()))


def _seq_and_batch(rows, splits=()):
    seq, fast = R.DualVertexSet(), R.DualVertexSet()
    idx_seq = [seq.push(v) for v in rows]
    idx_fast = np.concatenate([fast.push_batch(b) for b in np.array_split(rows, list(splits))])
    assert idx_fast.tolist() == idx_seq
    _same_sets(seq, fast)
    return np.array(idx_seq), seq


def test_key_restatement_basics():
    # splitmix64's first outputs from state 0 are mix64(0), mix64(golden), ... (public test vector)
    assert int(DC.mix64(0)[0]) == 0xE220A8397B1DCDAF
    assert int(DC.mix64(DC.GOLDEN)[0]) == 0x6E789E6AA1B965F4
    x = np.array([0.0, -0.0, 1 + 2.0 ** -16, 1.0, np.inf, np.nan, 5e-324])
    cb = DC.comp_bits(x)
    assert cb[0] == cb[1] == 0 and cb[2] == cb[3] == DC.bits(np.array([1.0]))[0]
    assert cb[4] == DC.bits(np.array([np.inf]))[0] and cb[5] == DC.bits(np.array([np.nan]))[0] and cb[6] == 1
    P = np.array([[1.0, -2.0, 0.0], [1.0, -2.0, -0.0], [-2.0, 1.0, 0.0], [1.0, np.nan, 0.0]])
    h, f, nan = DC.key(P)
    assert h.tolist()[:3] == [R.hash_dual_vector(v) for v in P[:3]] and nan.tolist() == [False, False, False, True]
    assert f[0] == f[1] and f[0] != f[2] and h[0] == h[2]                  # the position enters the fingerprint
    want = DC.mix64(np.uint64((sum(int(DC.mix64(int(DC.comp_bits(P[0, i:i + 1])[0]) ^ ((DC.POS_MULT * (i + 1)) & DC.MASK64))[0])
                                   for i in range(3)) & DC.MASK64) ^ int(h[0])))
    assert f[0] == want[0]
    assert DC.digest([]) == 0 and DC.digest([5]) == (DC.GOLDEN + 5) & DC.MASK64
    assert DC.digest([5, 7]) == (2 * DC.GOLDEN + 5 + 3 * 7) & DC.MASK64 != DC.digest([7, 5])


def test_edge_values_round_as_claimed():
    E = DC.EDGE_VALUES
    for a, b in DC.EDGE_EQUAL:
        assert R.round16(E[a]) == R.round16(E[b]) and DC.bits(np.array(E[a])) != DC.bits(np.array(E[b])), (a, b)
    for a, b in DC.EDGE_APART:
        assert R.round16(E[a]) != R.round16(E[b]), (a, b)
    # the ties go to even, not up: floor(x + 0.5) would give 1 + 2^-15 and 2^17 + 4
    assert R.round16(E["1+2^-16"]) == 1.0 and R.round16(E["1+3*2^-16"]) == 1 + 2.0 ** -14
    assert R.round16(E["2^17+2"]) == 2.0 ** 17 and R.round16(E["2^17+6"]) == 2.0 ** 17 + 8
    assert R.round16(E["2-2^-17"]) == 2.0                                   # the carry
    # the scale 2^digits is finite up to digits = 1023 (|x| >= 2^-1008); below, x is kept
    for name in ("2^-1009", "2^-1009(1+2^-20)", "+min", "-min", "+max", "-max", "+inf", "-inf", "+0", "-0"):
        assert DC.bits(np.array(R.round16(E[name]))) == DC.bits(np.array(E[name])), name
    assert R.round16(E["2^-1008(1+2^-20)"]) == 2.0 ** -1008 and R.round16(E["2^-1007(1+2^-17)"]) == 2.0 ** -1007
    assert R.round16(E["1.7e308"]) != 1.7e308 and np.isfinite(R.round16(E["1.7e308"]))
    vals = np.array(list(E.values()))
    assert np.array_equal(DC.bits(R.round16_vec(vals)), DC.bits(np.array([R.round16(v) for v in vals])))


@pytest.mark.parametrize("m", EDGE_MS)
def test_edge_rows(m):
    E = DC.edge_rows(m)
    assert E.rows.shape[1] == m and E.positions == sorted({0, 63, 64, m - 1} & set(range(m)))
    for p in E.positions:
        for name, val in DC.EDGE_VALUES.items():
            assert DC.bits(E.rows[E.index[(p, name)], p]) == DC.bits(np.array(val))
    idx, ref = _seq_and_batch(E.rows, E.splits)
    _seq_and_batch(E.rows[::-1])
    at = lambda *k: int(idx[E.index[k]])
    for a, b in DC.EDGE_APART:
        for p in E.positions:
            assert at(p, a) != at(p, b), (p, a, b)
    # round16-equal components are one vertex where the hashes agree too: always at m = 1 (the hash
    # is the component's own rounding), and for every pair at one position at least
    merged = {(a, b): [p for p in E.positions if at(p, a) == at(p, b)] for a, b in DC.EDGE_EQUAL}
    print(f"m = {m}: {len(ref)} vertices of {len(E.rows)} rows; merges {merged}")
    assert all(merged.values()), merged
    for p in E.positions:                                  # +0.0 is pushed first and is the vertex kept
        assert at(p, "+0") == at(p, "-0") and DC.bits(ref.data[at(p, "+0")][p]) == 0
    nan_rows = np.flatnonzero(np.isnan(E.rows).any(axis=1))
    assert len(set(idx[nan_rows].tolist())) == len(nan_rows) >= len(E.positions)      # each its own vertex
    if m >= 2:
        h = R.hash_dual_rows(E.rows)
        inf_bits = DC.bits(np.array([np.inf]))[0]
        o = [E.index[("overflow", f)] for f in (1.0, 1 - 2.0 ** -10, 1 - 2.0 ** -30)]
        assert (h[o] == inf_bits).all() and np.isfinite(E.rows[o]).all()
        assert idx[o[0]] != idx[o[1]] and idx[o[0]] == idx[o[2]]
        i1, i2, i3 = (E.index[("inf", a, b)] for a, b in ((np.inf, 1.0), (np.inf, 2.0), (-np.inf, 1.0)))
        assert h[i1] == h[i2] == h[i3] == inf_bits and len({idx[i1], idx[i2], idx[i3]}) == 3
        t0, t1 = E.index[("twin", "-0")], E.index[("twin", "+0")]
        assert t0 < t1 and idx[t0] == idx[t1] and DC.bits(ref.data[idx[t0]][E.positions[-1]]) == DC.bits(np.array(-0.0))
    assert (idx[E.n_first:] < idx[:E.n_first].max() + 1).sum() >= 20      # the repeats find old vertices (NaN ones append)


@pytest.mark.parametrize("m", PAIR_MS)
def test_hash_split_pairs(m):
    H = DC.hash_split_pairs(m)
    assert H.split.shape == H.mirror.shape == (8, 2, m)
    for a, b in H.split:
        assert np.array_equal(b, a * (1 + 2.0 ** -18))
        assert all(R.round16(x) == R.round16(y) for x, y in zip(a, b)) and R.hash_dual_vector(a) != R.hash_dual_vector(b)
    for a, b in H.mirror:
        assert sum(R.round16(x) != R.round16(y) for x, y in zip(a, b)) == 1 and R.hash_dual_vector(a) == R.hash_dual_vector(b)
    rows = DC.pair_rows(H)
    idx, ref = _seq_and_batch(rows, [1, 5, 16])
    assert idx.tolist() == list(range(32)) + list(range(0, 32, 2))        # every pair is two vertices


@pytest.mark.parametrize("m", WRAP_MS)
def test_wrap_rows(m):
    W = DC.wrap_rows(m)
    home = DC.key(W)[1] & np.uint64(DC.TCAP0 - 1)
    print(f"m = {m}: {len(W)} wrap rows of 20000, {int((home == DC.TCAP0 - 1).sum())} on the last slot")
    assert len(W) >= 16 and (home >= DC.TCAP0 - 2).all() and not np.isnan(W).any()
    F = DC.wrap_filler(m, W)
    ref = R.DualVertexSet()
    assert ref.push_batch(np.vstack([F, W])).tolist() == list(range(len(F) + len(W)))   # all distinct
    # the third push of the GPU test, [W, WRAP_AGAIN filler rows], stays at the table's growth threshold
    T = DC.host_trace([("push", len(F), 0), ("push", len(W), len(F)), ("push", len(W) + DC.WRAP_AGAIN, len(F) + len(W))])
    assert T[2].need == DC.TCAP0 // 2 and [e.tcap for e in T] == [DC.TCAP0] * 3 and len(F) >= 200
    # the batch table of a push of count <= 512 rows has TCAP0 slots too
    assert [e.tt for e in T] == [DC.TCAP0] * 3


@pytest.mark.parametrize("m", CONTENTION_MS)
def test_contention_batch(m):
    B = DC.contention_batch(m)
    n = len(B.rows)
    assert n == 40000 > DC.MAX_WAVES and 0.003 * n <= len(B.nan) <= 0.007 * n
    ref = R.DualVertexSet()
    idx = ref.push_batch(B.rows)
    assert len(ref) == B.nbase + len(B.nan)
    clean = np.setdiff1d(np.arange(n), B.nan)
    first = {b: int(clean[B.pick[clean] == b][0]) for b in range(B.nbase)}
    late = [b for b in range(B.nbase) if first[b] > DC.MAX_WAVES]
    assert len(late) == B.nlate >= 5
    for b in range(B.nbase):                               # every row finds the first row of its base vector
        rows_b = clean[B.pick[clean] == b]
        assert (idx[rows_b] == idx[first[b]]).all() and np.array_equal(DC.bits(ref.data[idx[first[b]]]), DC.bits(B.rows[first[b]]))
    assert (B.nan < DC.MAX_WAVES).any() and (B.nan > DC.MAX_WAVES).any()
    assert 0.15 * n <= (DC.bits(B.rows[clean]) != DC.bits(B.base[B.pick[clean]])).any(axis=1).sum() <= 0.35 * n
    again = ref.push_batch(B.rows)                         # onto the full set: found, but for the NaN rows
    assert np.array_equal(again[clean], idx[clean]) and again[B.nan].tolist() == list(range(len(ref) - len(B.nan), len(ref)))


@pytest.mark.parametrize("m", GROWTH_MS)
def test_growth_script(m):
    steps = DC.growth_script(m)
    ref = R.DualVertexSet()
    sizes, ops = [], []
    for s in steps:
        before = len(ref)
        if s.op == "push":
            assert s.rows.shape[1] == m
            idx = ref.push_batch(s.rows)
            if len(s.rows) > 1 and before:
                assert (idx < before).any() and (idx >= before).any(), s.note          # old and new in every batch
            ops.append(("push", len(s.rows), before))
        else:
            assert s.size <= before and (s.op == "truncate" or s.size == 0)
            kept = ref.matrix(m)[:s.size]
            ref = R.DualVertexSet()
            if s.size:
                ref.push_batch(kept)
            ops.append((s.op, 0, before))
        assert len(ref) == s.size_after, s.note
        sizes.append(len(ref))
    assert [511, 512, 513] == sizes[3:6]
    assert [s.size for s in steps if s.op != "push"] == [600, 300, 1, 0, 0] and steps[-2].op == "clear"
    T = DC.host_trace(ops)
    assert [e.count for e in T[:9]] == [1, 255, 54, 256, 2, 2, 255, 1024, 1025] and 2049 in [e.count for e in T]
    assert [(e.need, e.cap_grew, e.cap) for e in T[:3]] == [(1, True, 256), (256, False, 256), (257, True, 768)]
    assert [(e.need, e.table_grew, e.tcap) for e in T[3:5]] == [(512, False, 1024), (513, True, 2048)]
    assert (T[6].need, T[6].cap_grew) == (768, False)
    assert T[7].cap_grew and T[7].table_grew and (T[7].cap, T[7].tcap) == (1792, 4096) and not T[7].ws_grew and T[7].tt == 2048
    assert T[8].ws_grew and T[8].cap_grew and (T[8].cap, T[8].tt) == (3840, 4096)
    big = next(e for e in T if e.count == 2049)
    assert big.ws_grew and big.tt_grew and big.tt == 8192 and big.table_grew and big.tcap == 8192
    assert [e.ws_grew for e in T].count(True) == 3 and [e.table_grew for e in T].count(True) == 4
    assert any(np.isnan(s.rows).any() for s in steps if s.op == "push")
