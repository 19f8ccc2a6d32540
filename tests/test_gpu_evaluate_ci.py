"""Out-of-sample evaluation with a confidence interval on the device: eval_moments_kernel through
twosd_moments_of_values, the stream estimators twosd_evaluate_moments / _paired / _ci and the
two-rank evaluate_ci_sharded.

Reference: the C oracle's objectives on the same Philox stream (cpu.sample_deltas +
CpuLP.solve_batch), their moments taken in np.longdouble; HiGHS for the bounded template.
Tolerances: the moments step itself 1e-12 relative on mean and m2 (emulated error of the blockwise
two-pass + merge scheme: <= 7e-16); on 1e6 + N(0,1) data (1 / cv = 1e6) m2 to 1e-9 -- ten times
the a-priori scale 2^-53 / cv = 1.1e-10, three orders below the best case of the one-pass formula
sum v^2 - n mean^2 (1.9e-6).  Against the oracle the LP's own 1e-9 objective tolerance dominates:
mean to 1e-9 (1 + |mean|), variance to 1e-6 relative."""
import copy
import functools
import os
import struct

import numpy as np
import pytest

from tests import bounds_cases as BC
from tests import instances as I

pytestmark = pytest.mark.gpu

SEED = 777


class _env:
    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        self.old = os.environ.get(self.key)
        os.environ[self.key] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop(self.key, None)
        else:
            os.environ[self.key] = self.old


def _ld(v):
    """(n, mean, m2, min, max) of v, the sums in long double."""
    v = np.asarray(v, dtype=np.longdouble)
    mean = v.sum() / v.size
    return int(v.size), float(mean), float(((v - mean) ** 2).sum()), float(v.min()), float(v.max())


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def _bytes(m):
    return struct.pack("<qqdddd", m.n, m.n_bad, m.mean, m.m2, m.min, m.max)


@functools.lru_cache(maxsize=None)
def _ctx(name):
    """One context per instance for the whole file: basis at x_EV, distributions uploaded."""
    from sqlp_amd import smps, twosd
    inst = I.load(name)
    ctx = twosd.SDContext(inst["sp2"], inst["sto"])
    x = I.x_ev(name)
    ctx.compute_basis(x, smps.mean_values(inst["sto"]))
    ctx.set_distributions(inst["sto"])
    return ctx, x


def _x_b(name):
    x = I.x_ev(name)
    return x * (1.0 + 0.1 * np.random.default_rng(4).uniform(0.8, 1.2, size=x.shape))


@functools.lru_cache(maxsize=None)
def _oracle(name, N, which="a"):
    """The oracle's objectives of scenarios [0, N) of stream SEED at x_EV ("a") or _x_b ("b")."""
    from oracle import cpu
    ctx, x = _ctx(name)
    if which == "b":
        x = _x_b(name)
    sp = I.load(name)["osp2"]
    deltas = cpu.sample_deltas(I.load(name)["sto"], ctx.positions, ctx.template_values, N, SEED)
    lp = cpu.CpuLP(sp.W, sp.q, sp.senses)
    lp.set_basis(ctx.get_basis())
    obj, _, _, st, _ = lp.solve_batch(ctx.rows, sp.r - sp.T @ x, deltas, nthreads=8)
    assert (st == 0).all()
    obj.setflags(write=False)
    return obj


def _check_vs_oracle(m, ref_obj, tag):
    n, mean, m2, mn, mx = _ld(ref_obj)
    var = m2 / (n - 1)
    print(f"{tag}: n {m.n} mean {m.mean!r} (oracle {mean!r}, rel {_rel(m.mean, mean):.2e}) "
          f"variance rel {_rel(m.variance, var):.2e} min/max {m.min!r} {m.max!r}")
    assert (m.n, m.n_bad) == (n, 0)
    assert abs(m.mean - mean) <= 1e-9 * (1 + abs(mean))
    assert _rel(m.variance, var) <= 1e-6
    assert abs(m.min - mn) <= 1e-9 * (1 + abs(mn)) and abs(m.max - mx) <= 1e-9 * (1 + abs(mx))


def _agree(a, b, tol=1e-12):
    assert (a.n, a.n_bad) == (b.n, b.n_bad)
    assert abs(a.mean - b.mean) <= tol * (1 + abs(b.mean))
    assert abs(a.m2 - b.m2) <= tol * (1 + abs(b.m2))
    assert a.min == b.min and a.max == b.max


# ---- 1. the kernel's shapes, through moments_of_values ---------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 65537])
def test_kernel_shapes_conditioning(N):
    """1e6 + N(0,1): one value per block (N <= 256), a block of two next to blocks of one and
    empty blocks (257), slices of 257 with a short last one (65537)."""
    from sqlp_amd import twosd
    ctx, _ = _ctx("lands")
    v = 1e6 + np.random.default_rng(N).normal(size=N)
    m = twosd.moments_of_values(ctx, v)
    n, mean, m2, mn, mx = _ld(v)
    print(f"N {N}: mean rel err {_rel(m.mean, mean):.2e}, m2 rel err {_rel(m.m2, m2):.2e}")
    assert (m.n, m.n_bad, m.min, m.max) == (N, 0, mn, mx)
    assert abs(m.mean - mean) <= 1e-12 * abs(mean)
    if N == 1:
        assert m.m2 == 0.0
    else:
        assert abs(m.m2 - m2) <= 1e-9 * m2
    assert _bytes(twosd.moments_of_values(ctx, v)) == _bytes(m)          # the same bits on every run
    # well-conditioned data: the moments step itself to 1e-12
    w = 250.0 + 40.0 * np.random.default_rng(N + 1).normal(size=N)
    mw = twosd.moments_of_values(ctx, w, np.zeros(N, dtype=np.int32))
    _, mean, m2, _, _ = _ld(w)
    assert abs(mw.mean - mean) <= 1e-12 * abs(mean) and abs(mw.m2 - m2) <= 1e-12 * m2


@pytest.mark.parametrize("N", [3, 257, 65537])
def test_kernel_constant_array_is_exact(N):
    from sqlp_amd import twosd
    ctx, _ = _ctx("lands")
    m = twosd.moments_of_values(ctx, np.full(N, 174.65))       # no power of two: n * c rounds
    assert (m.n, m.mean, m.m2, m.min, m.max) == (N, 174.65, 0.0, 174.65, 174.65)


@pytest.mark.parametrize("N", [255, 257, 65537])
def test_kernel_status_mask(N):
    """One entry in seven not optimal and NaN: never read into a sum, a minimum or a maximum."""
    from sqlp_amd import twosd
    ctx, _ = _ctx("lands")
    v = 1e6 + np.random.default_rng(N + 2).normal(size=N)
    st = np.zeros(N, dtype=np.int32)
    st[3::7] = np.array([1, 2, 3])[np.arange(len(st[3::7])) % 3]
    v[st != 0] = np.nan
    m = twosd.moments_of_values(ctx, v, st)
    n, mean, m2, mn, mx = _ld(v[st == 0])
    assert (m.n, m.n_bad, m.min, m.max) == (n, int((st != 0).sum()), mn, mx)
    assert np.isfinite([m.mean, m.m2]).all()
    assert abs(m.mean - mean) <= 1e-12 * abs(mean) and abs(m.m2 - m2) <= 1e-9 * m2
    # a whole slice of the first blocks masked: their records are identities
    st2 = np.zeros(N, dtype=np.int32)
    st2[: N // 2] = 1
    v2 = np.where(st2 != 0, np.nan, 1e6 + np.arange(N) % 5)
    m2_ = twosd.moments_of_values(ctx, v2, st2)
    n, mean, m2, mn, mx = _ld(v2[st2 == 0])
    assert (m2_.n, m2_.n_bad, m2_.min, m2_.max) == (n, N // 2, mn, mx)
    assert abs(m2_.mean - mean) <= 1e-12 * abs(mean) and abs(m2_.m2 - m2) <= 1e-9 * m2


def test_kernel_all_masked_and_empty():
    from sqlp_amd import twosd
    ctx, _ = _ctx("lands")
    m = twosd.moments_of_values(ctx, np.full(1000, np.nan), np.full(1000, 2, dtype=np.int32))
    assert (m.n, m.n_bad, m.mean, m.m2, m.min, m.max) == (0, 1000, 0.0, 0.0, np.inf, -np.inf)
    e = twosd.moments_of_values(ctx, np.zeros(0))
    assert (e.n, e.n_bad, e.mean, e.m2, e.min, e.max) == (0, 0, 0.0, 0.0, np.inf, -np.inf)


# ---- 2. stream moments against the oracle ----------------------------------------------------------
@pytest.mark.parametrize("name,N", [("lands", 20000), ("transship", 20000), ("storm", 8192)])
def test_stream_moments_match_oracle(name, N):
    from sqlp_amd import twosd
    ctx, x = _ctx(name)
    zero = np.zeros(len(x))
    m = twosd.evaluate_moments(ctx, zero, x, SEED, 0, N)
    _check_vs_oracle(m, _oracle(name, N), name)
    s2 = twosd.evaluate_sampled(ctx, zero, x, N, SEED)
    assert abs(m.mean * N / N - s2) <= 1e-12 * (1 + abs(s2)), (m.mean, s2)
    assert twosd.evaluate_moments(ctx, zero, x, SEED, 0, N) == m         # the same bits on every run
    with _env("TWOSD_EVAL_CHUNK", "4096"):
        _agree(twosd.evaluate_moments(ctx, zero, x, SEED, 0, N), m)
    a = 7777
    parts = twosd.evaluate_moments(ctx, zero, x, SEED, 0, a).merge(twosd.evaluate_moments(ctx, zero, x, SEED, a, N - a))
    _agree(parts, m)
    # a shard's share of the evaluate sum, and c'x inside mean / min / max
    sa = twosd.evaluate_sampled(ctx, zero, x, N, SEED, 0, a)
    ma = twosd.evaluate_moments(ctx, zero, x, SEED, 0, a)
    assert abs(ma.mean * a / N - sa) <= 1e-12 * (1 + abs(sa))
    c1 = np.linspace(1.0, 2.0, len(x))
    mc = twosd.evaluate_moments(ctx, c1, x, SEED, 0, a)
    cx = float(c1 @ x)
    assert (mc.mean, mc.min, mc.max, mc.m2) == (ma.mean + cx, ma.min + cx, ma.max + cx, ma.m2)


# ---- 3. non-optimal scenarios ----------------------------------------------------------------------
def test_non_optimal_scenarios_are_counted_out():
    """lands with a demand (70, probability 0.1) no capacity covers: TWOSD_E_LP, those scenarios in
    n_bad, the moments over the others."""
    from oracle import cpu
    from sqlp_amd import smps, twosd
    from sqlp_amd._lib import TwoSDError
    inst = I.load("lands")
    sto = copy.deepcopy(inst["sto"])
    (pos, (kind, support, probs)), = sto.indep.items()
    assert kind == "DISCRETE" and max(support) == 7.0
    sto.indep[pos] = ("DISCRETE", list(support) + [70.0], [0.9 * p for p in probs] + [0.1])
    ctx = twosd.SDContext(inst["sp2"], sto)
    x = I.x_ev("lands")
    ctx.compute_basis(x, smps.mean_values(inst["sto"]))
    ctx.set_distributions(sto)
    N = 4096
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, N, SEED)
    vals = twosd.get_scenarios(epi)
    bad = vals[:, 0] == 70.0
    assert 300 < bad.sum() < 520
    zero = np.zeros(len(x))
    with pytest.raises(TwoSDError) as ei:
        twosd.evaluate_moments(ctx, zero, x, SEED, 0, N)
    assert ei.value.code == -4
    sp = inst["osp2"]
    lp = cpu.CpuLP(sp.W, sp.q, sp.senses)
    lp.set_basis(ctx.get_basis())
    o_obj, _, _, o_st, _ = lp.solve_batch(ctx.rows, sp.r - sp.T @ x, vals - ctx.template_values, nthreads=4)
    assert ((o_st != 0) == bad).all()
    n, mean, m2, mn, mx = _ld(o_obj[~bad])
    with _env("TWOSD_EVAL_CHUNK", "1000"):                     # every chunk still runs
        for m in (twosd.evaluate_moments(ctx, zero, x, SEED, 0, N, raise_on_status=False),
                  twosd.evaluate_ci(ctx, zero, x, SEED, batch=1024, n_max=N, rel_tol=0.0, raise_on_status=False).moments):
            assert (m.n, m.n_bad) == (n, int(bad.sum()))
            assert abs(m.mean - mean) <= 1e-9 * (1 + abs(mean)) and _rel(m.m2, m2) <= 1e-6
            assert abs(m.min - mn) <= 1e-9 * (1 + abs(mn)) and abs(m.max - mx) <= 1e-9 * (1 + abs(mx))


# ---- 4. bounded template: c0 inside mean, min and max ----------------------------------------------
def test_bounded_template_moments():
    from sqlp_amd import smps, twosd
    inst, sp2, osp2, hp = BC.lands()
    ctx = twosd.SDContext(sp2, inst["sto"])
    ctx.compute_basis(BC.lands_xs()[0], smps.mean_values(inst["sto"]))
    ctx.set_distributions(inst["sto"])
    x = BC.lands_xs()[3]
    N = 2048
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, N, SEED)
    ref = BC.lands_highs(3, twosd.get_scenarios(epi))
    m = twosd.evaluate_moments(ctx, np.zeros(ctx.n1), x, SEED, 0, N)
    _check_vs_oracle(m, ref, "bounded lands")


# ---- 5. paired -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lands", "storm"])
def test_paired_on_common_random_numbers(name):
    from sqlp_amd import twosd
    ctx, xa = _ctx(name)
    xb = _x_b(name)
    N = 4096
    zero = np.zeros(len(xa))
    a, b, d = twosd.evaluate_paired(ctx, zero, xa, xb, SEED, 0, N)
    assert a == twosd.evaluate_moments(ctx, zero, xa, SEED, 0, N)
    assert b == twosd.evaluate_moments(ctx, zero, xb, SEED, 0, N)
    oa, ob = _oracle(name, N, "a"), _oracle(name, N, "b")
    _check_vs_oracle(a, oa, name + " a")
    _check_vs_oracle(b, ob, name + " b")
    n, mean, m2, mn, mx = _ld(oa.astype(np.longdouble) - ob.astype(np.longdouble))
    scale = 1 + max(np.abs(oa).max(), np.abs(ob).max())
    print(f"{name}: diff mean {d.mean!r} (oracle {mean!r}) m2 rel {_rel(d.m2, m2):.2e}; variance of the difference / "
          f"(var a + var b) = {d.variance / (a.variance + b.variance):.3e} (common random numbers' gain)")
    assert d.n == a.n == b.n == N and d.n_bad == 0
    assert abs(d.mean - mean) <= 2e-9 * scale
    assert _rel(d.m2, m2) <= 1e-6
    assert abs(d.min - mn) <= 2e-9 * scale and abs(d.max - mx) <= 2e-9 * scale
    with _env("TWOSD_EVAL_CHUNK", "1500"):
        a2, b2, d2 = twosd.evaluate_paired(ctx, zero, xa, xb, SEED, 0, N)
    _agree(a2, a)
    _agree(b2, b)
    assert abs(d2.mean - d.mean) <= 1e-12 * scale and _rel(d2.m2, d.m2) <= 1e-12


# ---- 6. the sequential rule ------------------------------------------------------------------------
Z = 1.96
BATCH = 1024


def _oracle_rule(obj, rel_tol, offset=0.0, batch=BATCH):
    """(stopping n, half-width there, converged) of the rule on the oracle's objectives, after
    asserting that no checkpoint's half-width lies within 2 % of its threshold."""
    for n in range(batch, len(obj) + 1, batch):
        cnt, mean, m2, _, _ = _ld(obj[:n])
        hw = Z * float(np.sqrt(m2 / (cnt - 1) / cnt))
        thr = rel_tol * abs(offset + mean)
        assert abs(hw - thr) > 0.02 * thr, (n, hw, thr)
        if hw <= thr:
            return n, hw, True
    return len(obj), hw, False


@pytest.mark.parametrize("name,rel_tol,n_max", [("lands", 0.009, 6144), ("ssn", 0.02, 6144)])
def test_sequential_rule_stops_where_the_oracle_stops(name, rel_tol, n_max):
    from sqlp_amd import twosd
    ctx, x = _ctx(name)
    zero = np.zeros(len(x))
    obj = _oracle(name, n_max)
    n_stop, hw, conv = _oracle_rule(obj, rel_tol)
    assert conv and BATCH < n_stop < n_max                     # the case separates: not the first batch, not the cap
    r = twosd.evaluate_ci(ctx, zero, x, SEED, batch=BATCH, n_max=n_max, rel_tol=rel_tol, z=Z)
    print(f"{name}: stops at n = {r.n}, half-width {r.half_width!r} (oracle {hw!r}), mean {r.mean!r}")
    assert (r.n, r.n_bad, r.converged) == (n_stop, 0, True)
    assert _rel(r.half_width, hw) <= 1e-6
    assert r.half_width == Z * r.moments.std_error or _rel(r.half_width, Z * r.moments.std_error) <= 1e-15
    _agree(r.moments, twosd.evaluate_moments(ctx, zero, x, SEED, 0, n_stop))


def test_sequential_rule_cap_and_clipped_batch():
    from sqlp_amd import twosd
    ctx, x = _ctx("ssn")
    zero = np.zeros(len(x))
    r = twosd.evaluate_ci(ctx, zero, x, SEED, batch=BATCH, n_max=3072, rel_tol=1e-3, z=Z)
    assert (r.n + r.n_bad, r.converged) == (3072, False)
    assert r.half_width > 1e-3 * abs(r.mean)
    ctx, x = _ctx("lands")
    zero = np.zeros(len(x))
    r = twosd.evaluate_ci(ctx, zero, x, SEED, batch=1000, n_max=2500, rel_tol=1e-6, z=Z)
    assert (r.n + r.n_bad, r.converged) == (2500, False)       # batches of 1000, 1000 and 500
    _agree(r.moments, twosd.evaluate_moments(ctx, zero, x, SEED, 0, 2500))
    first = twosd.evaluate_ci(ctx, zero, x, SEED, batch=1000, n_max=2500, rel_tol=1e-6, z=Z, first=500)
    _agree(first.moments, twosd.evaluate_moments(ctx, zero, x, SEED, 500, 2500))


def test_sequential_rule_offset_enters_the_threshold():
    """lands, first batch: half-width = 0.0166 |mean| > 0.009 |mean|, so offset 0 goes on; with
    offset = c'x = 2 mean the threshold is 0.009 * 3 |mean| and the rule stops at n = 1024."""
    from sqlp_amd import twosd
    ctx, x = _ctx("lands")
    obj = _oracle("lands", 6144)
    mean1 = float(np.mean(obj[:BATCH]))
    c1 = np.zeros(len(x))
    c1[0] = 2.0 * mean1 / x[0]
    offset = float(c1 @ x)
    n0, _, _ = _oracle_rule(obj, 0.009)
    n1, hw1, conv = _oracle_rule(obj, 0.009, offset=offset)
    assert (n1, conv) == (BATCH, True) and n0 > BATCH
    r = twosd.evaluate_ci(ctx, c1, x, SEED, batch=BATCH, n_max=6144, rel_tol=0.009, z=Z)
    assert (r.n, r.converged) == (BATCH, True) and _rel(r.half_width, hw1) <= 1e-6
    assert abs(r.mean - (offset + mean1)) <= 1e-9 * (1 + abs(offset + mean1))
    # abs_tol alone stops it as well: max(abs_tol, rel_tol |.|)
    r = twosd.evaluate_ci(ctx, np.zeros(len(x)), x, SEED, batch=BATCH, n_max=6144, rel_tol=0.0, abs_tol=1.5 * hw1, z=Z)
    assert (r.n, r.converged) == (BATCH, True)


# ---- 7. two ranks on one GPU -----------------------------------------------------------------------
def _ci_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sqlp_amd import dist as sdist
        ctx, x = _ctx("lands")
        out[rank] = sdist.evaluate_ci_sharded(ctx, np.zeros(len(x)), x, SEED, batch=BATCH, n_max=6144, rel_tol=0.009, z=Z)
    finally:
        dist.destroy_process_group()


def test_two_ranks_take_the_same_stop_decision():
    """evaluate_ci_sharded on two ranks sharing cuda:0 over gloo (the layout of
    tests/test_gpu_dist.py): both ranks return the same bits, stop where one rank stops, and the
    mean agrees to the merge's rounding."""
    import torch.multiprocessing as mp
    from sqlp_amd import twosd
    from tests.test_gpu_dist import _free_port
    port = _free_port()
    with mp.get_context("spawn").Manager() as mgr:
        out = mgr.dict()
        mp.start_processes(_ci_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
        res = dict(out)
    ctx, x = _ctx("lands")
    one = twosd.evaluate_ci(ctx, np.zeros(len(x)), x, SEED, batch=BATCH, n_max=6144, rel_tol=0.009, z=Z)
    assert res[0] == res[1]
    assert (res[0].n, res[0].n_bad, res[0].converged) == (one.n, one.n_bad, True)
    assert abs(res[0].mean - one.mean) <= 1e-12 * (1 + abs(one.mean))
    assert _rel(res[0].half_width, one.half_width) <= 1e-12
