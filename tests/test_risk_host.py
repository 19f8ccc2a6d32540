"""Host side of the mean-CVaR recourse (no GPU):

* sqlp_amd/csrc/risk_keys.h (the order-preserving key and the exact threshold ceil(level Q)) in a
  stand-alone program (tests/native/risk_check.cpp) built by the host compiler with ASan + UBSan
  (`make sanitize_risk`) and run directly, against the Python restatement;
* the restated quantile (tests/risk_ref.py) against a brute-force sort on the directed inputs;
* the master row of a tail cut on lands and on lands3b, from the oracle's picks and scores, against
  the sample's E[(h - eta)+] with h from the CPU LP;
* the RiskCell master algebra on a hand-made two-cut case, using qp_solve only.
"""
import os
import shutil
import struct
import subprocess
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from tests import instances as I
from tests import risk_cases as RC
from tests import risk_ref as RR

ROOT = I.ROOT


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _run_native(args):
    if shutil.which("make") is None or shutil.which("c++") is None:
        pytest.skip("make / c++ not available")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sqlp_amd", "csrc"), "sanitize_risk"])
    exe = os.path.join(ROOT, "sqlp_amd", "csrc", "build_san", "risk_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return [line.split() for line in r.stdout.splitlines()]


def test_native_keys_match_the_restatement_and_order():
    vals = [0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, 1.5, 1.5000000000000002, -1e308, 1e308, float("inf"), float("-inf"),
            2.2250738585072014e-308, -3.25]
    out = _run_native(["key"] + [f"{_bits(v):016x}" for v in vals])
    assert len(out) == len(vals)
    keys = []
    for v, line in zip(vals, out):
        assert line[0] == "key" and int(line[1], 16) == _bits(v)
        assert int(line[2], 16) == RR.key(v)
        assert int(line[3], 16) == _bits(v)                      # the round trip gives the bits back
        keys.append(int(line[2], 16))
    order = sorted(range(len(vals)), key=lambda i: keys[i])
    sv = [vals[i] for i in order]
    assert all(a <= b for a, b in zip(sv, sv[1:]))                # numeric order
    assert RR.key(-0.0) + 1 == RR.key(0.0)                        # -0 directly before +0


def test_native_threshold_is_exact():
    rng = np.random.default_rng(5)
    cases = [(0.5, 7), (0.5, 8), (0.9, 10), (0.9, 1), (1 - 2.0 ** -20, 1 << 20), (1 - 2.0 ** -20, (1 << 20) + 1),
             (0.1, (1 << 58) + 12345), (5e-324, 3), (2.0 ** -60, 1 << 63), (1 - 2.0 ** -53, (1 << 64) - 1), (0.3, (1 << 64) - 1)]
    cases += [(float(rng.uniform(0.001, 0.999)), int(rng.integers(1, 1 << 62))) for _ in range(40)]
    args = ["thr"]
    for level, Q in cases:
        args += [f"{_bits(level):016x}", Q]
    out = _run_native(args)
    assert len(out) == len(cases)
    for (level, Q), line in zip(cases, out):
        want = RR.threshold(level, Q)
        assert int(line[3]) == want, (level, Q)
        assert 1 <= want <= Q and Fraction(level) * Q <= want < Fraction(level) * Q + 1


@pytest.mark.parametrize("n", RC.SIZES)
def test_restated_quantile_against_a_plain_sort(n):
    seen_exact = seen_fraction = False
    for name, (vals, w, st) in RC.directed(n).items():
        for level in RC.LEVELS:
            got = RR.quantile(vals, w, st, level)
            assert got is not None, name
            var, cvar, tail_q, Q, n_bad = got
            ok = np.ones(n, dtype=bool) if st is None else (np.asarray(st) == 0)
            q = [1] * n if w is None else RR.int_weights(w)
            qk = [q[s] for s in range(n) if ok[s]]
            vk = np.asarray(vals)[ok]
            assert Q == sum(qk) and n_bad == n - int(ok.sum())
            assert var == RR.brute_quantile(vk, qk, level), (name, level)    # == : -0 and +0 compare equal here
            t = RR.threshold(level, Q)
            below = sum(qq for v, qq in zip(vk, qk) if RR.key(v) <= RR.key(var))
            strictly = sum(qq for v, qq in zip(vk, qk) if RR.key(v) < RR.key(var))
            assert strictly < t <= below and tail_q == Q - below
            # Rockafellar-Uryasev: cvar = var + E[(v - var)+] / (1 - level), at least var, at most the maximum
            assert var <= cvar <= max(float(vk.max()), var) + 1e-9 * (1 + abs(var)) or tail_q == 0
            if tail_q == 0:
                assert cvar == var
            seen_exact |= name == "exact_hit" and level == 0.5 and below == t and n >= 3
            seen_fraction |= (Fraction(level) * Q).denominator != 1
            if name == "zeros":
                n_neg = (n + 1) // 2                                          # entries 0, 2, ... are -0
                want_neg = t <= n_neg
                assert np.signbit(var) == want_neg, (n, level)
    assert seen_fraction
    assert seen_exact or n < 3


# ---- the master row of a tail cut, from the oracle's picks and scores ------------------------------
def _instance(name):
    """(oracle stage-2 template of lands' core, rows of the random elements, N x k values)."""
    from sqlp_amd import smps
    inst = I.load("lands")
    if name == "lands":
        sto = inst["sto"]
    else:
        _, _, sto = smps.load_smps(os.path.join(I.DATA, name))
    _, rows, cols = smps.scenario_positions(inst["sp2"], sto)
    assert (cols < 0).all()
    vals = smps.sample_values(sto, 48, np.random.default_rng(17))
    return inst["osp2"], rows, vals


@pytest.mark.parametrize("name", ["lands", "lands3b"])
def test_tail_row_bounds_the_sample_excess_from_below(name):
    from oracle import cpu
    sp, rows, vals = _instance(name)
    N = len(vals)
    xb = I.x_ev("lands")
    rng = np.random.default_rng(3)
    w = rng.uniform(0.5, 2.0, size=N)
    W = float(w.sum())
    DR = vals - sp.r[rows]
    lp = cpu.CpuLP(sp.W, sp.q, sp.senses)
    st, _, head, _ = lp.solve_from_slack(sp.r - sp.T @ xb)
    assert st == 0
    lp.set_basis(head)

    def h(x):
        obj, pi, _, s, _ = lp.solve_batch(rows, sp.r - sp.T @ x, DR, nthreads=1)
        assert (s == 0).all()
        return obj, pi

    hb, pib = h(xb)
    _, pi2 = h(1.25 * xb)
    V = np.unique(np.round(np.vstack([pib, pi2]), 12), axis=0)
    _, _, mv, ma = cpu.build_cut(sp.r, sp.T, xb, V, rows, DR, w, tie_rel=0.0, nthreads=1)
    np.testing.assert_allclose(mv, hb, rtol=1e-9, atol=1e-9)             # V holds every scenario's optimal dual at xb
    cols = -np.ones(len(rows), dtype=np.int64)
    for eta_b in (float(np.quantile(mv, 0.7)), float(mv.min()) - 1.0, float(np.sort(mv)[N // 2])):
        a_t, b_t, W_t = RR.tail_cut(sp.r, sp.T, 0.0, rows, cols, V, DR, w, ma, mv, eta_b)
        assert W_t == pytest.approx(float(w[mv > eta_b].sum()), rel=1e-14)
        d = W_t / W
        grid = [(xb, eta_b), (1.2 * xb, eta_b), (xb + np.array([1.0, 0.0, 0.5, 0.0]), eta_b - 20.0),
                (1.5 * xb, eta_b + 15.0), (xb, eta_b + 40.0), (xb, eta_b - 40.0)]
        for x, eta in grid:
            hx, _ = h(x)
            ref = float(w @ np.maximum(hx - eta, 0.0)) / W
            row = d * (a_t + float(b_t @ x) - eta)
            assert row <= ref + 1e-8 * (1 + abs(ref)), (name, eta_b, x, eta, row, ref)
        # at the build point the row is the argmax form of the sample's excess
        ref = float(w @ np.maximum(mv - eta_b, 0.0)) / W
        row = d * (a_t + float(b_t @ xb) - eta_b)
        assert abs(row - ref) <= 1e-8 * (1 + abs(ref)), (name, eta_b, row, ref)


# ---- RiskCell master algebra on a hand-made case ---------------------------------------------------
def _hand_cell(lam=0.5, level=0.8):
    from sqlp_amd import master, risk, smps, twosd
    inst = I.load("lands")
    sp1 = smps.get_smps_stage_template(inst["cor"], inst["tim"], 1)
    cell = risk.RiskCell(sp1, None, risk.MeanCVaR(level, lam))
    epi = SimpleNamespace(objective_weight=1.0, lower_bound=0.0, total_scenario_weight=10.0,
                          cuts=[twosd.sdCut(400.0, np.array([-20.0, -15.0, -10.0, -12.0]), 8.0)],
                          incumbent_cut=twosd.sdCut(330.0, np.array([-12.0, -9.0, -7.0, -8.0]), 10.0))
    cell.bind_epigraph(epi)
    t1 = twosd.sdTailCut(520.0, np.array([-25.0, -18.0, -12.0, -15.0]), 3.0, 8.0, 300.0)
    t2 = twosd.sdTailCut(450.0, np.array([-16.0, -12.0, -9.0, -10.0]), 2.5, 10.0, 280.0)
    cell.tail_cuts.append(risk.tail_row(t1, 8.0))
    cell.tail_incumbent = risk.tail_row(t2, 10.0)
    x0 = I.x_ev("lands")
    cell.x_candidate, cell.x_incumbent = x0.copy(), x0.copy()
    cell.eta_candidate = cell.eta_incumbent = 280.0
    cell.add_regularization(x0, 280.0, 0.1)
    return cell, epi, (t1, t2), x0, sp1


def test_risk_cell_rows_and_master():
    from sqlp_amd import master
    lam, level = 0.5, 0.8
    cell, epi, (t1, t2), x0, sp1 = _hand_cell(lam, level)
    var, alpha, beta = cell.master_rows()
    np.testing.assert_array_equal(var, [0, 0, 1, 1])
    # mean rows: aged by 8 / 10, then the incumbent; no eta term
    np.testing.assert_allclose(alpha[:2], [0.8 * 400.0, 330.0], rtol=1e-15)
    np.testing.assert_allclose(beta[0], np.append(0.8 * epi.cuts[0].beta, 0.0), rtol=1e-15)
    np.testing.assert_allclose(beta[1], np.append(epi.incumbent_cut.beta, 0.0), rtol=1e-15)
    # tail rows: d (alpha + beta'x - eta), aged by 8 / 10, then the incumbent's with d = 2.5 / 10
    d1, d2 = 3.0 / 8.0, 0.25
    np.testing.assert_allclose(alpha[2:], [0.8 * d1 * 520.0, d2 * 450.0], rtol=1e-15)
    np.testing.assert_allclose(beta[2], 0.8 * d1 * np.append(t1.beta, -1.0), rtol=1e-15)
    np.testing.assert_allclose(beta[3], d2 * np.append(t2.beta, -1.0), rtol=1e-15)
    assert cell.weights() == ((1 - lam) * 1.0, lam / (1 - level))
    x, eta = cell.solve_master()
    # the same master assembled by hand: z = (x, eta, m, tau)
    n1 = 4
    c1 = np.asarray(sp1.q, dtype=np.float64)
    A1, b1 = sp1.dense_W(), np.asarray(sp1.r, dtype=np.float64)
    H = np.array([0.1] * 5 + [0.0, 0.0])
    g = np.concatenate([c1 - 0.1 * x0, [lam - 0.1 * 280.0, 1 - lam, lam / (1 - level)]])
    Aeq, beq, G, h = master._split_rows(np.hstack([A1, np.zeros((A1.shape[0], 3))]), b1, list(sp1.sense))
    Gc = np.zeros((4, 7))
    Gc[:, :5] = beta
    Gc[[0, 1], 5] = -1.0
    Gc[[2, 3], 6] = -1.0
    Gb, hb = master._bound_rows(sp1.ylb, sp1.yub, 7)
    Gt = np.zeros((1, 7)); Gt[0, 6] = -1.0
    res = master.qp_solve(H, g, Aeq, beq, np.vstack([G, Gc, Gb, Gt]), np.concatenate([h, -alpha, hb, [0.0]]))
    assert res.status == master.OPTIMAL
    np.testing.assert_allclose(np.append(x, eta), res.z[:5], rtol=1e-9, atol=1e-9)
    # at the optimum both epigraph variables sit on their rows, and the objective is the composite one
    z = np.append(x, eta)
    m = max(alpha[0] + beta[0] @ z, alpha[1] + beta[1] @ z)
    tau = max(0.0, alpha[2] + beta[2] @ z, alpha[3] + beta[3] @ z)
    want = float(c1 @ x) + lam * eta + (1 - lam) * m + lam / (1 - level) * tau + 0.05 * float((z - np.append(x0, 280.0)) @ (z - np.append(x0, 280.0)))
    assert cell.master_obj == pytest.approx(want, rel=1e-7)
    # the composite epigraph values check_improvement reads are the same rows
    from sqlp_amd import twosd
    comp = cell.composite()
    assert twosd.evaluate_multi_epigraph(comp, z) == pytest.approx((1 - lam) * m + lam / (1 - level) * tau, rel=1e-12)
    # cut removal: a tail cut whose multiplier is small leaves, the incumbent rows stay
    cell._mean_duals, cell._tail_duals = np.array([0.5]), np.array([0.0])
    cell.remove_cuts_by_multiplier()
    assert len(epi.cuts) == 1 and cell.tail_cuts == [] and cell.tail_incumbent is not None


def test_risk_interface_refusals():
    from sqlp_amd import risk
    for level, lam in ((0.0, 0.5), (1.0, 0.5), (0.8, -0.1), (0.8, 1.5)):
        with pytest.raises(ValueError):
            risk.MeanCVaR(level, lam)
    assert risk.MeanCVaR(0.8, 1.0).value(10.0, 3.0, 2.0) == pytest.approx(3.0 + 2.0 / 0.2)
    assert risk.MeanCVaR(0.8, 0.0).value(10.0, 3.0, 2.0) == 10.0
    cell, epi, _, _, _ = _hand_cell()
    with pytest.raises(ValueError, match="one epigraph"):
        cell.bind_epigraph(epi)
    with pytest.raises(ValueError, match="feasibility"):
        risk.sd_run(cell, lambda i: [], 1, feasibility=True)
    with pytest.raises(TypeError, match="stop"):
        risk.sd_run(cell, lambda i: [], 1, stop=None)
