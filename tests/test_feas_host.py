"""Feasibility rays on the host (no GPU): twosd_fray_key, the cell's feasibility rows and the
master with them, and the library's new symbols."""
import ctypes

import numpy as np
import pytest

from tests import feas_cases as FC


def _key(v):
    from sqlp_amd import twosd
    return twosd.fray_key(np.asarray(v, dtype=np.float64))


def test_fray_key_scaling_flip_and_rounding():
    rng = np.random.default_rng(3)
    for mv in (1, 5, 64, 65, 130):
        v = rng.normal(size=mv) * (rng.uniform(size=mv) < 0.6)
        v[rng.integers(mv)] = 2.5
        k0, n0 = _key(v)
        assert np.abs(n0).max() == 1.0
        np.testing.assert_array_equal(n0, v / np.abs(v).max())
        for sc in (2.0, 0.125, 3.0, 1e-7, 1e9):                            # invariant under positive scaling
            assert _key(sc * v)[0] == k0
        i = int(np.flatnonzero(v)[0])
        w = v.copy()
        w[i] = -w[i]
        assert _key(w)[0] != k0                                            # a flipped component
        if mv > 1:
            j = int(np.flatnonzero(np.abs(v) < 2.5)[0]) if (np.abs(v) < 2.5).any() else None
            if j is not None and v[j] != 0:
                w = v.copy()
                w[j] *= 1.0 + 2.0 ** -30                                   # below the 24-bit rounding
                assert _key(w)[0] == k0 and not np.array_equal(_key(w)[1], n0)
                w[j] = v[j] * (1.0 + 2.0 ** -20)                           # above it
                assert _key(w)[0] != k0


def test_fray_key_refuses_zero_and_non_finite_rays():
    from sqlp_amd._lib import TwoSDError
    for bad in ([0.0, 0.0, 0.0], [0.0, -0.0], [1.0, np.nan], [np.inf, 1.0], [1e-300 * 0.0]):
        with pytest.raises(TwoSDError) as e:
            _key(bad)
        assert e.value.code == -1


def test_new_symbols_exist_in_the_library():
    from sqlp_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = ["twosd_solve_rays", "twosd_feas_scan", "twosd_fray_push", "twosd_fray_size", "twosd_fray_get", "twosd_fray_clear",
             "twosd_fray_key", "twosd_last_ray_stats"]
    assert all(hasattr(lib, n) for n in names)
    bound = {n for n, _, _ in _lib.SIGNATURES}
    assert set(names) <= bound
    assert _lib.FRAY_MAX == 4096


class _Ctx:
    """What sdCell needs of a context on the host."""
    lib = None


def _cell(with_epi=True):
    from sqlp_amd import master
    L = FC.lands3f()
    cell = master.sdCell(L.sp1, _Ctx())
    if with_epi:
        cell.bind_epigraph(type("E", (), dict(objective_weight=1.0, lower_bound=0.0, cuts=[], incumbent_cut=None))())
    return cell, L


def test_add_feasibility_row_dedup():
    cell, _ = _cell()
    b = np.array([-1.0, -1.0, -1.0, -1.0])
    assert cell.add_feasibility_row(14.0, b) is True
    assert cell.add_feasibility_row(14.0, b.copy()) is False               # equal in alpha and beta
    assert cell.add_feasibility_row(14.0, b * (1 + 2.0 ** -52)) is True    # any other bits: another row
    assert cell.add_feasibility_row(13.0, b) is True
    assert len(cell.feas_rows) == 3
    b[0] = 5.0                                                             # the cell keeps its own copy
    assert cell.feas_rows[0][1][0] == -1.0


def test_master_with_a_feasibility_row_equals_the_hand_built_qp():
    from sqlp_amd import master
    cell, L = _cell()
    x0 = L.x_ev
    cell.add_regularization(x0, 0.5)
    cuts = (np.array([0]), np.array([100.0]), np.array([[-10.0, -8.0, -6.0, -4.0]]))
    base, lam0, obj0 = cell.solve_master_rows(*cuts)
    assert base.status == master.OPTIMAL and base.z[:4].sum() < 13.9      # the cut alone does not ask for 14
    cell.add_feasibility_row(14.0, -np.ones(4))                            # 14 - sum(x) <= 0
    cell.feas_margin = 1e-6
    res, lam, obj = cell.solve_master_rows(*cuts)
    assert res.status == master.OPTIMAL
    # the hand-built system: stage-1 rows, the cut, the bounds, then the row with its margin
    n1, nz = 4, 5
    Aeq, beq, G, h = master._split_rows(np.hstack([cell.A1, np.zeros((cell.A1.shape[0], 1))]), cell.b1, cell.sense1)
    Gc = np.array([[-10.0, -8.0, -6.0, -4.0, -1.0]])
    Gb, hb = master._bound_rows(L.sp1.ylb, L.sp1.yub, nz)
    Gf = np.array([[-1.0, -1.0, -1.0, -1.0, 0.0]])
    hf = np.array([-14.0 - 1e-6 * 15.0])
    H = np.array([0.5] * 4 + [0.0])
    g = np.concatenate([cell.c1 - 0.5 * x0, [1.0]])
    ref = master.qp_solve(H, g, Aeq, beq, np.vstack([G, Gc, Gb, Gf]), np.concatenate([h, [-100.0], hb, hf]))
    np.testing.assert_array_equal(res.z, ref.z)
    np.testing.assert_array_equal(lam, ref.lam[G.shape[0]:G.shape[0] + 1])
    assert res.z[:4].sum() >= 14.0 + 1e-6 * 15.0 - 1e-8
    assert obj > obj0


def test_a_cell_without_rows_builds_the_same_matrices_as_before(monkeypatch):
    """With no feasibility row the QP handed to qp_solve is the one of the parent commit: stage-1
    rows, cut rows, bound rows, nothing else; and an epigraph without a cut still raises."""
    from sqlp_amd import master
    cell, L = _cell()
    cell.add_regularization(L.x_ev, 0.1)
    seen = {}

    def spy(H, g, A, b, G, h, **kw):
        seen.update(H=H, g=g, A=A, b=b, G=G, h=h)
        return master.QPResult(master.OPTIMAL, np.zeros(len(g)), np.zeros(len(b)), np.zeros(len(h)), 0.0, 0)

    monkeypatch.setattr(master, "qp_solve", spy)
    alpha, beta = np.array([100.0, 50.0]), np.array([[-10.0, -8.0, -6.0, -4.0], [1.0, 0.0, 0.0, 0.0]])
    cell.solve_master_rows(np.array([0, 0]), alpha, beta)
    Aeq, beq, G, h = master._split_rows(np.hstack([cell.A1, np.zeros((cell.A1.shape[0], 1))]), cell.b1, cell.sense1)
    Gc = np.hstack([beta, -np.ones((2, 1))])
    Gb, hb = master._bound_rows(L.sp1.ylb, L.sp1.yub, 5)
    np.testing.assert_array_equal(seen["G"], np.vstack([G, Gc, Gb]))
    np.testing.assert_array_equal(seen["h"], np.concatenate([h, -alpha, hb]))
    np.testing.assert_array_equal(seen["A"], Aeq)
    np.testing.assert_array_equal(seen["b"], beq)
    with pytest.raises(RuntimeError, match="master is unbounded"):
        cell.solve_master_rows(np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros((0, 4)))
    # with a feasibility row the same call fixes eta at the lower bound instead
    cell.add_feasibility_row(14.0, -np.ones(4))
    cell.solve_master_rows(np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros((0, 4)))
    assert seen["A"].shape[0] == Aeq.shape[0] + 1 and seen["A"][-1].tolist() == [0, 0, 0, 0, 1] and seen["b"][-1] == 0.0
    assert seen["G"].shape[0] == G.shape[0] + Gb.shape[0] + 1
