"""The integer (int8-limb) pass of the cut on the host: the numpy model's error stays inside the
band formula (sqlp_amd/csrc/cut_i8.h band_term, what cut_vbase_kernel folds), the limbs stay in
int8 at the extremes, and the shared header gives the model's numbers bit for bit (a stand-alone
program under ASan + UBSan, tests/native/cut_i8_check.cpp)."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import cut_i8_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
LS = [3, 4]


def _exact(pc, dv):
    """sum_e pc[v, e] dv[s, e] without rounding (rationals), as floats rounded once."""
    P = [[Fraction(float(a)) for a in row] for row in pc]
    out = np.zeros((len(dv), len(pc)))
    for s, drow in enumerate(dv):
        D = [Fraction(float(a)) for a in drow]
        for v, prow in enumerate(P):
            out[s, v] = float(sum(a * b for a, b in zip(prow, D)))
    return out


def _check_in_band(pc, dv, dmax, L, exact=None):
    t = M.scores(pc, dv, dmax, L).astype(np.float64)
    band = M.vertex_band(pc, dmax, L)
    exact = _exact(pc, dv) if exact is None else exact
    err = np.abs(t - exact)
    # the float() of the rational is within half an ulp of it
    assert (err <= band[None, :] + 2.0 ** -52 * np.abs(exact)).all(), float((err / np.maximum(band[None, :], 1e-300)).max())
    return float((err / np.maximum(band[None, :], 1e-300)).max())


def _fixture(name):
    from sqlp_amd import smps
    from tests import instances as I
    z = np.load(os.path.join(G, f"cut_{name}.npz"))
    inst = I.load(name)
    _, rows, cols = smps.scenario_positions(inst["sp2"], inst["sto"])
    x = z["x"]
    coef = np.where(cols < 0, 1.0, -x[np.maximum(cols, 0)])
    pc = z["V"][:, rows] * coef[None, :]
    dv = z["values"] - inst["osp2"].r[rows]
    return pc, dv


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("name", ["storm", "ssn"])
def test_fixture_errors_inside_the_band(name, L):
    pc, dv = _fixture(name)
    dv = dv[:24]
    dmax = np.abs(dv).max(axis=0)
    worst = _check_in_band(pc[:40], dv, dmax, L)
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("k", [1, 5, 64, 117, 128])
def test_random_wide_range_rows_inside_the_band(k, L):
    rng = np.random.default_rng(100 * L + k)
    pc = rng.normal(size=(12, k)) * 10.0 ** rng.uniform(-6, 6, size=(12, k)) * 10.0 ** rng.uniform(-20, 20, size=(12, 1))
    dv = rng.normal(size=(16, k)) * 10.0 ** rng.uniform(-6, 6, size=(1, k)) * 10.0 ** rng.uniform(-3, 0, size=(16, k))
    dv[0] = np.abs(dv).max(axis=0)                          # a scenario at dmax in every element
    dv[1] = -dv[0]
    _check_in_band(pc, dv, np.abs(dv).max(axis=0), L)


@pytest.mark.parametrize("L", LS)
def test_single_dominant_entry_and_zero_elements(L):
    rng = np.random.default_rng(L)
    k = 40
    pc = rng.normal(size=(6, k)) * 1e-9
    pc[:, 7] = [1e6, -1e6, 3.0, 2.0 ** 20, -(2.0 ** -30), 1.0]      # one dominant entry per row
    dv = rng.uniform(-1, 1, size=(10, k))
    dv[:, 3] = 0.0                                           # dmax_e = 0
    dv[:, 11] = 0.0
    dmax = np.abs(dv).max(axis=0)
    assert dmax[3] == 0.0
    _check_in_band(pc, dv, dmax, L)
    E, S, la = M.operands(pc, dmax, L)
    assert E[3] == M.E_MIN
    # an element whose deltas are all zero contributes nothing, whatever its vertex entry
    pc2 = pc.copy()
    pc2[:, 3] = 1e3
    t1, t2 = M.scores(pc, dv, dmax, L), M.scores(pc2, dv, dmax, L)
    # (the larger entry may change the vertex scale: compare against the exact value instead)
    _check_in_band(pc2, dv, dmax, L)
    assert np.isfinite(t1).all() and np.isfinite(t2).all()
    # all-zero deltas and all-zero vertices
    assert not M.scores(pc, np.zeros_like(dv), np.zeros(k), L).any()
    assert not M.scores(np.zeros_like(pc), dv, dmax, L).any()


@pytest.mark.parametrize("L", LS)
def test_limb_ranges_at_the_extremes(L):
    Q = M.kq(L)
    for E in (M.E_MIN, -1, 0, 1, 20, 100):
        sc = 2.0 ** E
        a = np.array([sc, -sc, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, np.nextafter(sc, 0), -np.nextafter(sc, 0),
                      sc / 3, -sc / 7, sc * 2.0 ** (-Q - 1), sc * 2.0 ** -Q, 1.5 * sc * 2.0 ** -Q])
        q = M.quantise(a, E, L)
        assert (np.abs(q) <= 2 ** Q).all() and q[0] == 2 ** Q and q[1] == -2 ** Q and not q[2:7].any()
        lb = M.limbs(q, L)
        assert (np.abs(lb) <= 64).all()
        assert lb[0].tolist() == [64] + [0] * (L - 1)
        back = np.zeros(len(q), dtype=np.int64)
        for l in range(L):
            back = back * 128 + lb[:, l]
        assert (back == q).all()
        assert M.scale_exp(sc) == E and M.scale_exp(np.nextafter(sc, np.inf)) == E + 1
    q = np.arange(-2 ** Q, 2 ** Q + 1, 37)
    lb = M.limbs(q, L)
    assert (np.abs(lb) <= 64).all() and (lb[:, 1:] >= -64).all() and (lb[:, 1:] <= 63).all()
    # level sums (at most L pairs, k = 128, limbs at +-64) convert to fp32 exactly and fit an int32
    assert 128 * L * 64 * 64 < 2 ** 24


def _build_check(L, tmp):
    cxx = shutil.which("clang++") or shutil.which("g++")
    exe = os.path.join(tmp, f"cut_i8_check_{L}")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", f"-DTWOSD_CUT_I8_L={L}", "-fsanitize=address,undefined",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "sqlp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "cut_i8_check.cpp"), "-o", exe])
    return exe


@pytest.mark.skipif(shutil.which("clang++") is None and shutil.which("g++") is None, reason="no host C++ compiler")
@pytest.mark.parametrize("L", LS)
def test_shared_header_equals_the_model_under_asan_ubsan(L, tmp_path):
    exe = _build_check(L, str(tmp_path))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    rng = np.random.default_rng(7 + L)
    cases = []
    for k, nv, N in [(1, 3, 5), (63, 9, 7), (65, 33, 4), (117, 31, 6), (128, 5, 9)]:
        pc = rng.normal(size=(nv, k)) * 10.0 ** rng.uniform(-4, 4, size=(nv, k)) * 10.0 ** rng.uniform(-10, 10, size=(nv, 1))
        dv = rng.normal(size=(N, k)) * 10.0 ** rng.uniform(-4, 4, size=(1, k))
        if k > 1:
            dv[:, k // 2] = 0.0
        cases.append((pc, dv))
    spc, sdv = _fixture("storm")
    cases.append((spc[:31], sdv[:8]))
    for i, (pc, dv) in enumerate(cases):
        dmax = np.abs(dv).max(axis=0)
        fin, fout = str(tmp_path / f"in{i}.bin"), str(tmp_path / f"out{i}.bin")
        with open(fin, "wb") as f:
            np.array([pc.shape[1], pc.shape[0], dv.shape[0]], dtype=np.int32).tofile(f)
            dmax.tofile(f)
            np.ascontiguousarray(pc).tofile(f)
            np.ascontiguousarray(dv).tofile(f)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
        nv, N = pc.shape[0], dv.shape[0]
        raw = np.fromfile(fout, dtype=np.uint8)
        t = raw[:4 * N * nv].view(np.float32).reshape(N, nv)
        band = raw[4 * N * nv:4 * N * nv + 8 * nv].view(np.float64)
        S = raw[4 * N * nv + 8 * nv:].view(np.int32)
        want = M.scores(pc, dv, dmax, L)
        assert np.array_equal(t.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(band, M.vertex_band(pc, dmax, L))
        assert np.array_equal(S, M.operands(pc, dmax, L)[1])
