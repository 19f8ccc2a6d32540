"""The tail cut and the cut's quantile (sqlp_amd/csrc/risk.hip: twosd_cut_tail, twosd_cut_quantile)
after a cut, against tests/risk_ref.tail_cut (boot_ref.reform with the counts 1[max_val > eta]) with
max_val and max_arg from the cut itself.

Instances: lands, and a generated template (tests/synth_cases.synth_template) with k = 70 random
elements (two per lane of the re-formation kernel), half of them technology-matrix entries, and
general bounds (a shifted and a boxed column: c0 != 0 and dual vectors longer than m2).
Tolerance: the project's cut tolerance 1e-8 (1 + |ref|), beta against its largest entry
(tests/test_gpu_bootstrap._close).  The tail weight is compared bit for bit with the integer-scaled
sum, which with these distinct random weights also pins the set of flagged scenarios.
Sizes: N in {1, 63, 64, 65} around one 64-scenario tile, 300 with several tiles and waves, and
lands at 2500: 40 tiles in 10 shards, where the shard-order sum of S has more terms than the
bootstrap's eight side-by-side segments (sqlp_amd/csrc/reform_layout.h, reform.hip)."""
import contextlib
import os
import struct

import numpy as np
import pytest

from tests import bounds_cases as BC
from tests import instances as I
from tests import risk_ref as RR
from tests import synth_cases as SC

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 300]
FIX = 2.0 ** 58


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = np.abs(ref).max(axis=-1, keepdims=True) if "beta" in what and ref.ndim else np.abs(ref)
    worst = (np.abs(got - ref) / (1e-8 * (1.0 + scale))).max(initial=0.0)
    print(f"{what}: worst error {worst:.3e} of the bound")
    assert worst <= 1.0, (what, worst)


def _k70_template(k=70):
    """synth_template's W, q and senses on (160, 400) with k random elements on k rows, RHS and T
    entries alternating (listed by descending row), the first structural column shifted (lb = 0.25)
    and the next two boxed."""
    B = SC.synth_template(160, 400, k, seed=170, amp=0.2)
    n1 = B.T.shape[1]
    elems = [(int(i), -1 if e % 2 == 0 else e % n1) for e, i in enumerate(B.rows)][::-1]
    lb, ub = B.lb.copy(), B.ub.copy()
    lb[0] = 0.25
    lb[1], ub[1] = 0.1, 0.9
    ub[2] = 1.5
    tmpl = np.array([B.r[i] if j < 0 else B.T[i, j] for i, j in elems])
    positions = [("RHS" if j < 0 else f"x{j}", f"r{i}") for i, j in elems]
    rng = np.random.default_rng(4170)
    u = rng.uniform(-1.0, 1.0, size=(300, k))
    vals = tmpl + np.where(np.array([j for _, j in elems]) < 0, B.amp, SC.T_AMP) * u
    return BC.stage_problem(B.W, B.T, B.q, B.r, B.sense, lb, ub), positions, vals


def _template_arrays(ctx):
    """(r, T, c0) of the LP the kernels solve: the canonical form's (tests/test_gpu_bootstrap.py)."""
    from sqlp_amd import twosd
    sp2 = ctx.sp2
    T = sp2.dense_T()
    cf = twosd.canonical_form(sp2.W, sp2.q, sp2.r, sp2.sense, sp2.ylb, sp2.yub)
    return np.asarray(cf.r), np.vstack([T, np.zeros((cf.m_lp - T.shape[0], T.shape[1]))]), cf.c0


_CTX = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c, *_ in _CTX.values():
        c.close()
    _CTX.clear()


def _context(name):
    """(ctx, x, values (300 x k), weights (300)), one context per instance for the module."""
    from sqlp_amd import smps, twosd
    if name not in _CTX:
        w = np.random.default_rng(21).uniform(0.5, 1.5, size=300)
        if name == "lands":
            inst = I.load("lands")
            ctx = twosd.SDContext(inst["sp2"], inst["sto"])
            x = I.x_ev("lands")
            ctx.compute_basis(x, smps.mean_values(inst["sto"]))
            vals = I.sample("lands", 300, 3)
        else:
            sp2, positions, vals = _k70_template()
            ctx = twosd.SDContext(sp2, positions=positions)
            x = SC.X[0]
            ctx.compute_basis(x, vals[0])
            assert ctx.k == 70 and ctx.mv > ctx.m and (ctx.cols >= 0).sum() == 35
        _CTX[name] = (ctx, x, vals, w)
    return _CTX[name]


def _cut(name, N, plant=False, data=None):
    """A fresh epigraph of the first N scenarios (of data = (values, weights) when given) with its cut
    at x: (B, epi, cut, max_val, max_arg)."""
    from types import SimpleNamespace
    from sqlp_amd import twosd
    ctx, x, vals, w = _context(name)
    if data is not None:
        vals, w = data
    vals, w = vals[:N].copy(), w[:N].copy()
    if plant and N >= 2:
        vals[1] = vals[0]                                  # two identical scenarios: one score, twice
    r, T, c0 = _template_arrays(ctx)
    V = twosd.sdDualVertexSet(ctx)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals, w)
    twosd.solve_push(epi, x, 0, N)
    cut, mv, ma = twosd._build_cut(epi, x, 0.0, want_argmax=True)
    B = SimpleNamespace(ctx=ctx, x=x, r=r, T=T, c0=c0, V=V, Vm=V.matrix(), dv=vals - ctx.template_values, w=w,
                        total=epi.total_scenario_weight)
    return B, epi, cut, mv, ma


def _check_tail(name, B, epi, mv, ma, eta, what):
    """cut_tail at eta against the restatement; returns the device result."""
    from sqlp_amd import twosd
    got = twosd.cut_tail(epi, eta)
    q = RR.int_weights(B.w, B.total)
    flags = mv > eta                                       # the flags: strict, on the scores the cut returned
    wunit = B.total / FIX
    assert _bits(got.tail_weight) == _bits(float(sum(qq for qq, f in zip(q, flags) if f)) * wunit), what
    assert _bits(got.total_weight) == _bits(float(sum(q)) * wunit), what
    a, b, W_t = RR.tail_cut(B.r, B.T, B.c0, B.ctx.rows, B.ctx.cols, B.Vm, B.dv, B.w, ma, mv, eta)
    _close(got.alpha, a, f"{what} alpha")
    _close(got.beta, b, f"{what} beta")
    _close(got.tail_weight, W_t, f"{what} tail weight")
    for blocks in ("1", "3"):
        with _env(TWOSD_RISK_BLOCKS=blocks):
            g2 = twosd.cut_tail(epi, eta)
        assert g2.alpha == got.alpha and g2.tail_weight == got.tail_weight and g2.total_weight == got.total_weight, (what, blocks)
        np.testing.assert_array_equal(g2.beta, got.beta)
    return got


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("name", ["lands", "k70"])
def test_tail_cut_matches_the_restatement(name, N):
    from sqlp_amd import twosd
    B, epi, cut, mv, ma = _cut(name, N, plant=True)
    if N >= 2:
        assert mv[0] == mv[1] and ma[0] == ma[1]           # the planted pair shares its score
    srt = np.sort(mv)
    # inside the sample
    _check_tail(name, B, epi, mv, ma, float(srt[(7 * N) // 10]), f"{name} N={N} eta at the 0.7 point")
    _check_tail(name, B, epi, mv, ma, 0.5 * float(srt[0] + srt[-1]), f"{name} N={N} eta mid-range")
    # below every score: the cut itself, d = 1
    lo = _check_tail(name, B, epi, mv, ma, float(srt[0]) - 1.0, f"{name} N={N} eta below")
    _close(lo.alpha, cut.alpha, f"{name} N={N} below: alpha against the cut")
    _close(lo.beta, cut.beta, f"{name} N={N} below: beta against the cut")
    assert lo.tail_weight == lo.total_weight and lo.d == 1.0
    _close(lo.total_weight, cut.weight_mark, f"{name} N={N} total weight")
    # above every score (and exactly the largest: strict): the zero cut with weight 0
    for eta in (float(srt[-1]) + 1.0, float(srt[-1])):
        hi = twosd.cut_tail(epi, eta)
        assert hi.alpha == 0.0 and not hi.beta.any() and hi.tail_weight == 0.0 and hi.d == 0.0
    # exactly the score the planted pair shares: strict > leaves both out
    got = _check_tail(name, B, epi, mv, ma, float(mv[0]), f"{name} N={N} eta at the planted score")
    q = RR.int_weights(B.w, B.total)
    assert got.tail_weight == float(sum(qq for qq, v in zip(q, mv) if v > mv[0])) * (B.total / FIX)


def test_tail_cut_past_eight_shards():
    """N = 2500: the S sums are added over 10 shards in shard order (one segment; the bootstrap's eight
    segments would add them in another order)."""
    N = 2500
    data = (I.sample("lands", N, 3), np.random.default_rng(22).uniform(0.5, 1.5, size=N))
    B, epi, cut, mv, ma = _cut("lands", N, data=data)
    _check_tail("lands", B, epi, mv, ma, float(np.sort(mv)[(7 * N) // 10]), f"lands N={N} eta at the 0.7 point")


@pytest.mark.parametrize("N", [1, 65, 300])
@pytest.mark.parametrize("name", ["lands", "k70"])
def test_cut_quantile_is_the_quantile_of_the_scores(name, N):
    from sqlp_amd import twosd
    B, epi, cut, mv, ma = _cut(name, N)
    for level in (0.5, 0.9, 1.0 - 2.0 ** -20):
        cq = twosd.cut_quantile(epi, level)
        qv = twosd.quantile_of_values(B.ctx, mv, level, weights=B.w)
        ref = RR.quantile(mv, B.w, None, level, total=B.total)
        assert _bits(cq.var) == _bits(qv.var) == _bits(ref[0]), (name, N, level)
        wunit = B.total / FIX
        assert cq.tail_weight == float(qv.tail_q) * wunit and cq.total_weight == float(qv.total_q) * wunit
        assert qv.tail_q == ref[2] and qv.total_q == ref[3]
        _close(cq.cvar, ref[1], f"{name} N={N} level={level} cvar")
        # the tail cut at eta = VaR weighs what the quantile reports above VaR
        assert twosd.cut_tail(epi, cq.var).tail_weight == cq.tail_weight
        with _env(TWOSD_RISK_BLOCKS="2"):
            c2 = twosd.cut_quantile(epi, level)
        assert c2 == cq


def test_state_errors_follow_picks_keep():
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    B, epi, cut, mv, ma = _cut("lands", 65)
    other = twosd.sdEpigraph(B.ctx, 1.0, 0.0)
    twosd.add_scenarios(other, I.sample("lands", 10, 5))
    twosd.build_sasa_cut(other, B.x, B.V, 0.0)
    for call in (lambda: twosd.cut_tail(epi, 0.0), lambda: twosd.cut_quantile(epi, 0.5)):
        with pytest.raises(TwoSDError, match="the last cut was built on epigraph") as e:
            call()
        assert e.value.code == -3
    assert twosd.cut_tail(other, -1.0).d == 1.0                               # the other epigraph's own cut is usable
    # an epigraph without scenarios takes the empty path
    empty = twosd.sdEpigraph(B.ctx, 1.0, 0.0)
    twosd.build_sasa_cut(empty, B.x, B.V, 0.0)
    with pytest.raises(TwoSDError, match="empty-epigraph path") as e:
        twosd.cut_tail(empty, 0.0)
    assert e.value.code == -3
    # clearing the vertex set invalidates the last cut
    twosd.build_sasa_cut(epi, B.x, B.V, 0.0)
    twosd.cut_tail(epi, 0.0)
    B.V.clear()
    for call in (lambda: twosd.cut_tail(epi, 0.0), lambda: twosd.cut_quantile(epi, 0.5)):
        with pytest.raises(TwoSDError, match="no cut to read the picks of") as e:
            call()
        assert e.value.code == -3
    with pytest.raises(TwoSDError) as e:
        twosd.cut_tail(epi, float("nan"))
    assert e.value.code in (-1, -3)
    with pytest.raises(ValueError):
        twosd.cut_quantile(epi, 1.0)


def test_k_128_is_refused():
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    B = SC.synth_template(160, 400, 128, seed=171, amp=0.2)
    ctx = twosd.SDContext(B.sp2, positions=B.positions)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    with pytest.raises(TwoSDError) as e:
        twosd.cut_tail(epi, 0.0)
    assert e.value.code == -5 and "127" in str(e.value)
    ctx.close()
