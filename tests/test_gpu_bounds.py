"""Stage-2 variables with general bounds (LO / UP / FX / FR / MI / boxed) on the GPU: the library
removes them by twosd_canonical_form and runs its kernels on the canonical LP; callers see y in
their own space, objectives of their own LP (the shift's constant c0 included) and dual vectors of
length mv = m2 + boxed variables.  Reference: HiGHS on the bounded LPs (oracle.lp_highs) and the
oracle's cut on the canonical template that tests/bounds_cases.canon_np builds.  Tolerances are
the project's: objectives 1e-9 relative (tests/test_gpu_lp.py), alpha / beta 1e-8 with max_arg
exact (tests/test_gpu_cut.py)."""
import os

import numpy as np
import pytest

from tests import bounds_cases as BC

pytestmark = pytest.mark.gpu


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


def _close(a, b, rel):
    np.testing.assert_allclose(a, b, rtol=rel, atol=rel)


# ---- 1. every kind ---------------------------------------------------------------------------------
def test_every_kind_toy():
    from sqlp_amd import twosd
    sp2 = BC.stage_problem(BC.TOY_W, BC.TOY_T, BC.TOY_Q, BC.TOY_R, BC.TOY_SENSE, BC.TOY_LB, BC.TOY_UB)
    ctx = twosd.SDContext(sp2, positions=[("RHS", f"r{i}") for i in range(3)])
    assert (ctx.m_lp, ctx.n_lp, ctx.n_bound_rows, ctx.mv) == (4, 6, 1, 4)
    vals = BC.toy_values(16)
    ctx.compute_basis(BC.TOY_X, BC.TOY_R)
    obj, y, pi, st = ctx.solve_values(BC.TOY_X, vals, want_pi=True, want_y=True)
    assert (st == 0).all() and y.shape == (16, 6) and pi.shape == (16, 4)
    B = vals - BC.TOY_T @ BC.TOY_X
    ref = BC.highs_objectives(BC.highs_problem(BC.TOY_W, BC.TOY_Q, BC.TOY_SENSE, BC.TOY_LB, BC.TOY_UB), B)
    print("toy obj", obj, "max rel err", np.abs(obj - ref).max() / np.abs(ref).max())
    _close(obj, ref, 1e-9)
    assert (y >= BC.TOY_LB - 1e-9).all() and (y <= BC.TOY_UB + 1e-9).all()
    assert (y[:, 4] == 1.5).all()
    _close(y @ BC.TOY_Q, obj, 1e-9)                                   # obj = q . y
    R = BC.canon_np(BC.TOY_W, BC.TOY_Q, BC.TOY_R, BC.TOY_SENSE, BC.TOY_LB, BC.TOY_UB)
    b_ext = np.hstack([B - BC.TOY_W @ R.s, np.tile(R.r[3:], (16, 1))])
    _close(np.einsum("ij,ij->i", pi, b_ext) + R.c0, obj, 1e-9)        # obj = v . b_ext + c0
    assert (pi[:, 3] <= 1e-12 * (1 + np.abs(BC.TOY_Q).max())).all()   # boxed multipliers <= 0
    assert (pi[:, 0] >= -1e-12).all() and (pi[:, 1] <= 1e-12).all()   # G / L row duals keep JuMP's signs


# ---- 2. lands with bounds --------------------------------------------------------------------------
def _lands_ctx():
    from sqlp_amd import smps, twosd
    inst, sp2, osp2, hp = BC.lands()
    ctx = twosd.SDContext(sp2, inst["sto"])
    ctx.compute_basis(BC.lands_xs()[0], smps.mean_values(inst["sto"]))
    return ctx


def test_lands_bounded_objectives():
    from tests import instances as I
    inst, sp2, osp2, hp = BC.lands()
    # the instance is what the issue describes: objectives at x_EV for demand 3 / 5 / 7
    t0 = BC.lands_highs_by_demand(0)
    assert [t0[3.0], t0[5.0], t0[7.0]] == pytest.approx([174.65, 266.1667, 360.6667], abs=1e-4)
    ctx = _lands_ctx()
    assert (ctx.m_lp, ctx.n_lp, ctx.n_bound_rows) == (ctx.m + 4, ctx.n2, 4)   # UP on a [0, inf) column boxes it
    vals = I.sample("lands", 192, seed=23)
    lb, ub = sp2.ylb, sp2.yub
    bounded = [0, 4, 8, 11, 5]
    for xi, x in enumerate(BC.lands_xs()):
        obj, y, pi, st = ctx.solve_values(x, vals, want_pi=True, want_y=True)
        assert (st == 0).all()
        ref = BC.lands_highs(xi, vals)
        print("lands x", xi, "max rel err", np.abs(obj - ref).max() / np.abs(ref).max())
        _close(obj, ref, 1e-9)
        assert (y >= lb - 1e-9).all() and (y <= ub + 1e-9).all()
        act = (np.abs(y[:, bounded] - lb[bounded]) <= 1e-9) & (lb[bounded] != 0)
        act |= np.abs(y[:, bounded] - ub[bounded]) <= 1e-9
        assert act.any(axis=1).all()                                  # a bound is active in every LP
        _close(y @ sp2.q, obj, 1e-9)


# ---- 3. cut ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie_rel", [0.0, 1e-12])
def test_lands_bounded_cut(tie_rel):
    from oracle import cpu
    from sqlp_amd import twosd
    from tests import instances as I
    inst, sp2, osp2, hp = BC.lands()
    ctx = _lands_ctx()
    xs = BC.lands_xs()
    N = 192
    vals = I.sample("lands", N, seed=29)
    w = np.random.default_rng(6).uniform(0.5, 1.5, size=N)
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals, w)
    for x in xs[:2]:
        _, st, _ = twosd.solve_push(epi, x, 0, N)
        assert (st == 0).all()
    V = twosd.sdDualVertexSet(ctx)
    Vm = V.matrix()
    assert Vm.shape[1] == ctx.mv == ctx.m + 4
    R = BC.canon_np(osp2.W, osp2.q, osp2.r, osp2.senses, sp2.ylb, sp2.yub)
    Tc = np.vstack([osp2.T, np.zeros((R.nb, osp2.T.shape[1]))])
    p = w / w.sum()
    means = [float(p @ BC.lands_highs(xi, vals)) for xi in range(4)]
    cut, mv, ma = twosd._build_cut(epi, xs[2], tie_rel, want_argmax=True)
    a, b, omv, oma = cpu.build_cut(R.r, Tc, xs[2], Vm, ctx.rows, vals - osp2.r[ctx.rows], w, tie_rel=tie_rel, nthreads=4)
    print("cut alpha", cut.alpha, "oracle + c0", a + R.c0, "beta", cut.beta, b)
    assert (ma == oma).all()
    np.testing.assert_allclose(mv, omv + R.c0, rtol=1e-10, atol=1e-9)
    assert cut.alpha == pytest.approx(a + R.c0, rel=1e-8, abs=1e-8)
    np.testing.assert_allclose(cut.beta, b, rtol=1e-8, atol=1e-8 * (1 + np.abs(b).max()))
    # a valid lower bound of the bounded recourse at every x', and tight where the duals were pushed
    for xp, mean in zip(xs, means):
        assert cut.alpha + float(cut.beta @ xp) <= mean + 1e-8 * (1 + abs(mean))
    tight = twosd.build_sasa_cut(epi, xs[0], V, tie_rel=tie_rel)
    for xp, mean in zip(xs, means):
        assert tight.alpha + float(tight.beta @ xp) <= mean + 1e-8 * (1 + abs(mean))
    assert tight.alpha + float(tight.beta @ xs[0]) == pytest.approx(means[0], rel=1e-8)


# ---- 4. the 64-row slot boundary ---------------------------------------------------------------------
SLOT_N = 2048
SLOT_X = [np.array([0.5, 1.0, 0.2, 0.7]), np.array([0.9, 0.4, 0.6, 0.1])]


def _slot_values():
    S = BC.slot_template()
    return S.r[S.rows] + np.random.default_rng(0).uniform(-1.0, 1.0, size=(SLOT_N, len(S.rows)))


def _slot_run():
    """compute_basis at x0, pool_refresh at x1, keyed solve_push at x1 -> (objectives, V, LP us)."""
    from sqlp_amd import twosd
    S = BC.slot_template()
    ctx = twosd.SDContext(S.sp2, positions=[("RHS", f"r{i}") for i in S.rows])
    assert (ctx.m_lp, ctx.n_bound_rows) == (70, 10) and ctx.n_lp == S.W.shape[1] + 1
    vals = _slot_values()
    ctx.compute_basis(SLOT_X[0], vals[0])
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, vals)
    assert ctx.pool_refresh(epi, SLOT_X[1], 0, 512, 64) >= 1
    obj, st, nv = twosd.solve_push(epi, SLOT_X[1], 0, SLOT_N)
    assert (st == 0).all()
    Vm = twosd.sdDualVertexSet(ctx).matrix()
    assert nv == len(Vm)
    return obj, Vm, ctx.timings_us()[0]


def test_slot_boundary_refresh_and_keyed_push():
    S = BC.slot_template()
    vals = _slot_values()
    obj, Vm, _ = _slot_run()
    B = np.tile(S.r - S.T @ SLOT_X[1], (SLOT_N, 1))
    B[:, S.rows] += vals - S.r[S.rows]
    ref = BC.highs_objectives_blocked(S.W, S.q, S.sense, S.lb, S.ub, B)
    print("slot max rel err", np.abs(obj - ref).max() / np.abs(ref).max(), "|V|", len(Vm))
    _close(obj, ref, 1e-9)
    # every pushed vertex is dual feasible for the canonical LP: reduced costs >= 0, boxed multipliers <= 0
    R = BC.canon_np(S.W, S.q, S.r, S.sense, S.lb, S.ub)
    assert Vm.shape[1] == 70
    tol = 1e-9 * (1 + np.abs(R.q).max())
    assert (R.q[None, :] - Vm @ R.W >= -tol).all()
    assert (Vm[:, 60:] <= tol).all()
    with _env("TWOSD_PUSH_ALL", "1"):
        obj2, Vm2, _ = _slot_run()
    assert np.array_equal(obj, obj2) and np.array_equal(Vm, Vm2)


# ---- 5. sums ---------------------------------------------------------------------------------------
def test_lands_bounded_sums_and_scenarios():
    from sqlp_amd import twosd
    inst, sp2, osp2, hp = BC.lands()
    ctx = _lands_ctx()
    ctx.set_distributions(inst["sto"])
    x = BC.lands_xs()[3]
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, 256, seed=77)
    vals = twosd.get_scenarios(epi)
    assert set(np.unique(vals)) <= {3.0, 5.0, 7.0}                    # the caller's values, not the shifted rhs
    ref = BC.lands_highs(3, vals)
    obj, _, _, st = twosd.solve_batch(epi, x, want_pi=False)
    assert (st == 0).all()
    _close(obj, ref, 1e-9)
    ws, wt = ctx.last_objective()
    assert wt == 256.0 and ws / wt == pytest.approx(ref.mean(), rel=1e-9)
    ev = twosd.evaluate_sampled(ctx, np.zeros(ctx.n1), x, 256, seed=77)
    assert ev == pytest.approx(ref.mean(), rel=1e-9)


# ---- 6. end to end ---------------------------------------------------------------------------------
def _extensive_x(sp1, sp2, scenario_rhs, probs):
    """The LP of oracle.lp_highs.extensive_form, solved for its first-stage x as well."""
    from scipy.optimize import linprog
    from oracle import lp_highs
    S = len(scenario_rhs)
    n1, n2 = sp1.W.shape[1], sp2.W.shape[1]
    m1, m2 = sp1.W.shape[0], sp2.W.shape[0]
    A = np.zeros((m1 + S * m2, n1 + S * n2))
    A[:m1, :n1] = sp1.W
    for s in range(S):
        A[m1 + s * m2:m1 + (s + 1) * m2, :n1] = sp2.T
        A[m1 + s * m2:m1 + (s + 1) * m2, n1 + s * n2:n1 + (s + 1) * n2] = sp2.W
    b = np.concatenate([sp1.r] + list(scenario_rhs))
    G, L, E, A_ub, b_ub, A_eq, b_eq = lp_highs._split(list(sp1.senses) + list(sp2.senses) * S, A, b)
    lb = np.concatenate([sp1.cur_lb] + [sp2.cur_lb] * S)
    ub = np.concatenate([sp1.cur_ub] + [sp2.cur_ub] * S)
    bounds = [(None if np.isinf(l) else l, None if np.isinf(u) else u) for l, u in zip(lb, ub)]
    c = np.concatenate([sp1.q] + [p * sp2.q for p in probs])
    res = linprog(c, A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=b_eq, bounds=bounds, method="highs")
    assert res.status == 0
    return float(res.fun), res.x[:n1]


def test_lands_bounded_end_to_end():
    from oracle import lp_highs
    from sqlp_amd import smps, twosd
    inst, sp2, osp2, hp = BC.lands()
    sp1 = inst["osp1"]
    pos, rows, cols = smps.scenario_positions(sp2, inst["sto"])
    _, support, probs = inst["sto"].indep[pos[0]]
    rhs = []
    for v in support:
        r = osp2.r.copy()
        r[rows[0]] = v
        rhs.append(r)
    ext = lp_highs.extensive_form(sp1, osp2, rhs, probs)
    ext2, xs = _extensive_x(sp1, osp2, rhs, probs)
    assert ext2 == pytest.approx(ext, rel=1e-9)
    ctx = twosd.SDContext(sp2, inst["sto"])
    ctx.compute_basis(xs, smps.mean_values(inst["sto"]))
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_scenarios(epi, np.array(support, dtype=np.float64)[:, None], np.array(probs))
    _, st, _ = twosd.solve_push(epi, xs, 0, 3)
    assert (st == 0).all()
    cut = twosd.build_sasa_cut(epi, xs, twosd.sdDualVertexSet(ctx), tie_rel=0.0)
    total = float(sp1.q @ xs) + cut.alpha + float(cut.beta @ xs)
    print("end to end", total, ext)
    assert total == pytest.approx(ext, rel=1e-8)


# ---- 7. envelope and no-op -------------------------------------------------------------------------
def test_envelope_counts_bound_rows_and_default_is_noop():
    from sqlp_amd import twosd
    from sqlp_amd._lib import TwoSDError
    from tests import instances as I
    m2 = 1000
    lb, ub = np.zeros(m2), np.full(m2, np.inf)
    ub[:100] = 1.0
    big = BC.stage_problem(np.eye(m2), np.zeros((m2, 1)), np.ones(m2), np.ones(m2), ["E"] * m2, lb, ub)
    with pytest.raises(TwoSDError) as ei:
        twosd.SDContext(big)
    assert ei.value.code == -5 and "1100" in str(ei.value) and "1000" in str(ei.value)
    inst = I.load("lands")
    ctx = twosd.SDContext(inst["sp2"], inst["sto"])
    assert (ctx.m_lp, ctx.n_lp, ctx.n_bound_rows) == (ctx.m, ctx.n2, 0) and ctx.mv == ctx.m
