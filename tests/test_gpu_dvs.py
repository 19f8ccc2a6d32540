"""GPU dual-vertex-set dedup (push!, dual_set.jl:84-94) vs the oracle's linear scan."""
import numpy as np
import pytest

from oracle import twosd_ref
from tests import dvs_cases as DC
from tests import instances as I
from tests import synth_cases as SC

pytestmark = pytest.mark.gpu


def _ctx(name):
    from sqlp_amd import twosd
    inst = I.load(name)
    return twosd.SDContext(inst["sp2"], inst["sto"])


def test_dual_set_kat_on_device():
    # test/dual_set_test.jl with the length-3 vectors (newsvendor has m2 = 3)
    from sqlp_amd import twosd
    ctx = _ctx("newsvendor")
    V = twosd.sdDualVertexSet(ctx)
    sizes = []
    for v in ([1., 2, 3], [1.0000000001, 2, 3], [4., 5, 6], [3., 2, 1]):
        twosd.push(V, np.array(v))
        sizes.append(len(V))
    assert sizes == [1, 1, 2, 3]
    with pytest.raises(ValueError):          # length mismatch: the device set has fixed m2
        V.push(np.array([4., 5, 6, 7]))
    V.clear()
    assert len(V) == 0
    idx = twosd.sdDualVertexSet(ctx).push_batch(np.array([[1., 2, 3], [1.0000000001, 2, 3], [4., 5, 6], [4., 5, 6],
                                                           [3., 2, 1], [-0.0, 1, 1], [0.0, 1, 1]]))
    assert idx.tolist() == [0, 0, 1, 1, 2, 3, 3]     # -0.0 == 0.0 in Julia's r1 != r2


def _candidates(m, rng, nbase=60, n=400):
    base = np.round(rng.normal(size=(nbase, m)) * rng.choice([1, 10, 1000], size=(nbase, 1)), 4)
    base[rng.random(size=base.shape) < 0.6] = 0.0
    picks = rng.integers(0, nbase, size=n)
    C = base[picks].copy()
    kind = rng.integers(0, 5, size=n)
    C[kind == 1] *= 1 + 1e-12                            # rounding-equal (almost always)
    C[kind == 2] += rng.normal(size=(np.sum(kind == 2), m)) * 1e-3   # different
    C[kind == 3, 0] = -C[kind == 3, 0]                   # sign flip of one component
    C[kind == 4] = C[kind == 4] * (1 + 2.0 ** -15)       # right at the 16-bit granularity
    return C


@pytest.mark.parametrize("name", ["ssn", "transship"])
def test_push_batches_match_linear_scan(name):
    ctx = _ctx(name)
    from sqlp_amd import twosd
    rng = np.random.default_rng(11)
    C = _candidates(ctx.m, rng)
    V = twosd.sdDualVertexSet(ctx)
    ref = twosd_ref.DualVertexSet()
    for blk in np.array_split(C, [1, 50, 51, 220]):      # batches of 1, 49, 1, 169, 180
        got = V.push_batch(blk)
        want = [ref.push(v) for v in blk]
        assert got.tolist() == want
    assert len(V) == len(ref)
    np.testing.assert_array_equal(V.matrix(), ref.matrix(ctx.m))


def test_nan_vectors_always_appended():
    from sqlp_amd import twosd
    ctx = _ctx("newsvendor")
    V = twosd.sdDualVertexSet(ctx)
    idx = V.push_batch(np.array([[np.nan, 1, 1], [np.nan, 1, 1], [1.0, 1, 1], [1.0, 1, 1]]))
    assert idx.tolist() == [0, 1, 2, 2]


def test_truncate_rebuilds_lookup():
    from sqlp_amd import twosd
    ctx = _ctx("transship")
    rng = np.random.default_rng(2)
    C = np.round(rng.normal(size=(30, ctx.m)), 3)
    V = twosd.sdDualVertexSet(ctx)
    V.push_batch(C)
    V.truncate(10)
    idx = V.push_batch(C)
    assert idx[:10].tolist() == list(range(10)) and idx[10:].tolist() == list(range(10, 30))


# ---- directed cases (tests/dvs_cases.py; their conditions are proved in tests/test_dvs_cases.py) ----
# All comparisons are exact: the returned indices, the size, the vertices bit for bit (a uint64 view,
# so that -0.0 and NaN count) and the digest against its restatement.  The reference is the oracle's
# push_batch; after a truncate, a fresh oracle set rebuilt from the kept rows.
TID_OF_M = {1: "a", 20: "c", 64: "d", 65: "e", 129: "g", 257: "i", 1024: "p"}
_CTX = {}


def _set(m):
    """The (emptied) vertex set of a context with m rows: a synth_cases template with no basis
    computed (the set needs the template alone); m = 3 is newsvendor."""
    from sqlp_amd import twosd
    if m not in _CTX:
        if m == 3:
            _CTX[m] = _ctx("newsvendor")
        else:
            S = SC.template(TID_OF_M[m])
            _CTX[m] = twosd.SDContext(S.sp2, positions=S.positions)
    assert _CTX[m].mv == m
    V = twosd.sdDualVertexSet(_CTX[m])
    V.clear()
    assert len(V) == 0 and V.fingerprint() == 0
    return V


def _same(V, ref, m):
    assert len(V) == len(ref)
    got, want = V.matrix(), ref.matrix(m)
    assert got.shape == want.shape and np.array_equal(DC.bits(got), DC.bits(want))
    assert V.fingerprint() == DC.set_digest(want)


def _push_ways(m, rows, splits):
    """rows as one batch, in several batches and one row at a time, each into an empty set:
    the oracle's indices and set every time."""
    ref = twosd_ref.DualVertexSet()
    want = ref.push_batch(rows).tolist()
    for cuts in ([], list(splits), list(range(1, len(rows)))):
        V = _set(m)
        got = np.concatenate([V.push_batch(b) for b in np.array_split(rows, cuts)])
        assert got.tolist() == want, cuts[:8]
        _same(V, ref, m)
    return ref


@pytest.mark.parametrize("m", sorted(TID_OF_M))
def test_key_restatement_against_device(m):
    """fp_0 of a one-vertex set, recovered from its digest (size * golden + fp_0), against the
    restated fingerprint: the key kernel (round16, comp_bits, the sequential hash, mix64) on
    every edge row and on the rows the wrap case is selected with."""
    E = DC.edge_rows(m)
    rows = np.vstack([E.rows[:E.n_first], DC.stream_rows(m, 40, seed=1)])
    _, fp, _ = DC.key(rows)
    V = _set(m)
    for v, f in zip(rows, fp.tolist()):
        V.clear()
        assert V.push_batch(v[None, :]).tolist() == [0] and len(V) == 1
        assert (V.fingerprint() - DC.GOLDEN) & DC.MASK64 == f, v[DC.edge_positions(m)]


@pytest.mark.parametrize("m", sorted(TID_OF_M))
def test_edge_rows(m):
    E = DC.edge_rows(m)
    _push_ways(m, E.rows, E.splits)
    _push_ways(m, E.rows[::-1].copy(), E.splits)          # 0.0 after -0.0, the repeats first


@pytest.mark.parametrize("m", [3, 20, 65])
def test_hash_split_and_mirror_pairs(m):
    rows = DC.pair_rows(DC.hash_split_pairs(m))
    ref = _push_ways(m, rows, [1, 5, 16])
    assert len(ref) == 32                                 # every pair is two vertices


@pytest.mark.parametrize("m", [20, 65])
def test_wrap_rows_probe_through_slot_0(m):
    W = DC.wrap_rows(m)
    ref = twosd_ref.DualVertexSet()
    V = _set(m)
    assert V.push_batch(W).tolist() == ref.push_batch(W).tolist() == list(range(len(W)))
    assert V.push_batch(W).tolist() == list(range(len(W)))             # every row is found again
    assert V.push_batch(W[::-1].copy()).tolist() == list(range(len(W)))[::-1]
    _same(V, ref, m)
    for v in W:                                                        # and alone (the set's table only)
        assert V.push_batch(v[None, :]).tolist() == ref.push_batch(v[None, :]).tolist()
    _same(V, ref, m)
    # on top of a table filled up to its growth threshold: the last push has size + count == 512,
    # so the table keeps its 1024 slots throughout
    F = DC.wrap_filler(m, W)
    ref = twosd_ref.DualVertexSet()
    V = _set(m)
    for blk in (F, W, np.vstack([W, F[:DC.WRAP_AGAIN]])):
        assert V.push_batch(blk).tolist() == ref.push_batch(blk).tolist()
    assert len(V) == len(F) + len(W) == DC.TCAP0 // 2 - len(W) - DC.WRAP_AGAIN
    _same(V, ref, m)


@pytest.mark.parametrize("m", [65, 257])
def test_growth_script(m):
    ref = twosd_ref.DualVertexSet()
    V = _set(m)
    for s in DC.growth_script(m):
        if s.op == "push":
            assert V.push_batch(s.rows).tolist() == ref.push_batch(s.rows).tolist(), s.note
        else:
            kept = ref.matrix(m)[:s.size]
            ref = twosd_ref.DualVertexSet()
            if s.size:
                ref.push_batch(kept)
            if s.op == "clear":
                V.clear()
            else:
                V.truncate(s.size)
        assert len(V) == s.size_after, s.note
        _same(V, ref, m)                                  # the whole matrix and the digest after every step


@pytest.mark.parametrize("m", [3, 20])
def test_contention_batch(m):
    B = DC.contention_batch(m)
    ref = twosd_ref.DualVertexSet()
    V = _set(m)
    assert np.array_equal(V.push_batch(B.rows), ref.push_batch(B.rows))
    assert len(V) == B.nbase + len(B.nan)
    _same(V, ref, m)
    again = V.push_batch(B.rows)                          # onto the full set: the NaN rows append again
    assert np.array_equal(again, ref.push_batch(B.rows))
    assert len(V) == B.nbase + 2 * len(B.nan)
    _same(V, ref, m)


def test_digest_semantics():
    """What sqlp_amd/dist.py relies on: equal for sets whose vertices are round16-equal, different
    in another order and at another size."""
    from sqlp_amd import twosd
    m = 20
    P = 10.0 * DC.stream_rows(m, 60, seed=4)
    Q = P * (1 + 2.0 ** -40)
    assert not np.array_equal(P, Q) and np.array_equal(DC.key(P)[1], DC.key(Q)[1])
    V = _set(m)
    S = SC.template(TID_OF_M[m])
    other = twosd.sdDualVertexSet(twosd.SDContext(S.sp2, positions=S.positions))     # a second context
    assert V.push_batch(P).tolist() == list(range(60))
    d = V.fingerprint()
    assert d == DC.set_digest(P) == DC.set_digest(Q)
    assert len(other) == 0 and other.fingerprint() == 0
    assert other.push_batch(Q).tolist() == list(range(60))
    assert other.fingerprint() == d and not np.array_equal(DC.bits(other.matrix()), DC.bits(V.matrix()))
    other.ctx.close()
    assert V.push_batch(Q).tolist() == list(range(60)) and V.fingerprint() == d        # found: unchanged
    assert np.array_equal(DC.bits(V.matrix()), DC.bits(P))
    V.push_batch(-P[:1])
    d61 = V.fingerprint()
    assert len(V) == 61 and d61 != d and d61 == DC.set_digest(np.vstack([Q, -P[:1]]))   # one more vertex
    V.truncate(60)
    assert V.fingerprint() == d
    swapped = P.copy()
    swapped[[7, 8]] = swapped[[8, 7]]
    V.clear()
    V.push_batch(swapped)
    assert len(V) == 60 and V.fingerprint() != d and V.fingerprint() == DC.set_digest(swapped)


def test_refusals_leave_the_set_unchanged():
    import ctypes as C
    from sqlp_amd._lib import ptr
    m = 20
    P = DC.stream_rows(m, 30, seed=6)
    V = _set(m)
    V.push_batch(P)
    ctx, lib = V.ctx, V.ctx.lib
    ref = twosd_ref.DualVertexSet()
    ref.push_batch(P)
    buf = np.full((40, m), 7.0)
    for first, count in ((-1, 1), (0, 31), (30, 1), (31, 0), (0, -1), (29, 2)):
        assert lib.twosd_dvs_get(ctx.h, first, count, ptr(buf)) == -1 and b"dvs_get" in lib.twosd_last_error()
        assert (buf == 7.0).all()
    assert lib.twosd_dvs_get(ctx.h, 30, 0, ptr(buf)) == 0 and lib.twosd_dvs_get(ctx.h, 29, 1, ptr(buf)) == 0    # inside
    assert np.array_equal(buf[0], P[29]) and (buf[1:] == 7.0).all()
    _same(V, ref, m)
    for size in (31, -1, 1 << 30):
        assert lib.twosd_dvs_truncate(ctx.h, size) == -1 and b"dvs_truncate" in lib.twosd_last_error()
        _same(V, ref, m)
    ns = C.c_int(-7)
    assert lib.twosd_dvs_push(ctx.h, 0, None, None, C.byref(ns)) == 0 and ns.value == 30     # a no-op that reports the size
    assert V.push_batch(np.zeros((0, m))).tolist() == []
    assert lib.twosd_dvs_push(ctx.h, -1, ptr(buf), None, C.byref(ns)) == -1
    assert lib.twosd_dvs_push(ctx.h, 1, None, None, C.byref(ns)) == -1
    for bad in (np.ones(m + 1), np.ones(m - 1), np.ones((2, m + 1))):
        with pytest.raises(ValueError):
            V.push_batch(bad)
    _same(V, ref, m)
    assert V.push_batch(P[::-1].copy()).tolist() == list(range(30))[::-1]       # and the set still works
