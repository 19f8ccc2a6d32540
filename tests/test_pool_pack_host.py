"""The pool's packing step (sqlp_amd/csrc/pool_pack.h: pool_pack_basis) on the CPU: a stand-alone
program that includes only that header (tests/native/pool_pack_check.cpp), built by the host compiler
with ASan + UBSan (`make sanitize_pack`) and run directly, packs two small bases into exactly-sized
arrays and prints them.  The expected arrays below were worked out by hand from the layout upload_pool
documents: hb = 4 head + type (-1 past m), basic = bit (j >> 6) of word (j & 63) per basic column j,
B^{-1} by rows (CSR) and by columns (CSC, rows ascending) with pointers absolute from `base` and
padded to MP + 1 with their last value, d0_j = q_j - pi0'a_j (0 for basic and padding columns; a
slack's column is e_i)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def arrays():
    if shutil.which("make") is None or shutil.which("c++") is None:
        pytest.skip("make / c++ not available")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sqlp_amd", "csrc"), "sanitize_pack"])
    exe = os.path.join(ROOT, "sqlp_amd", "csrc", "build_san", "pool_pack_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        head, _, body = line.partition(" :")
        case, name = head.split()
        conv = float if name in ("rv", "cv", "d0") else int
        out[case, name] = [conv(t) for t in body.split()]
    return out


def test_small_exact(arrays):
    """m = 3, n = 4, rows (E, G, L), MP = 64, CH = 1, base = 5.  Columns: y0..y3 (type 0), slacks 4 (E: 3),
    5 (G: 1), 6 (L: 2).  W = [2 0 2 0; 0 1 0 1; 1 1 0 0], q = (1, 5, 3, 4), head = (y0, y3, slack 6),
    B^{-1} = [.5 0 0; 0 1 0; -.5 0 1], pi0 = (.5, 4, 0)."""
    a = {n: v for (c, n), v in arrays.items() if c == "small"}
    assert a["hb"] == [0 * 4 + 0, 3 * 4 + 0, 6 * 4 + 2] + [-1] * 61
    assert a["basic"] == [1, 0, 0, 1, 0, 0, 1] + [0] * 57
    assert a["rp"] == [5, 6, 7, 9] + [9] * 61
    assert a["rc"] == [0, 1, 0, 2]
    assert a["rv"] == [0.5, 1.0, -0.5, 1.0]
    assert a["cp"] == [5, 7, 8, 9] + [9] * 61        # column 0: rows 0, 2; column 1: row 1; column 2: row 2
    assert a["ci"] == [0, 2, 1, 2]
    assert a["cv"] == [0.5, -0.5, 1.0, 1.0]
    # y1: 5 - (4 * 1 + 0 * 1); y2: 3 - .5 * 2; slack of row 0: -.5; of row 1: -4; basic and padding: 0
    assert a["d0"] == [0.0, 1.0, 2.0, 0.0, -0.5, -4.0, 0.0] + [0.0] * 57


def test_two_lane_slots(arrays):
    """m = 65, n = 2: MP = 128 (R = 2), CH = 2, base = 7.  head[i] = slack 2 + i except head[3] = y0;
    rows 0 / 64 are E / G, the rest L; B^{-1} = I plus -4 at (64, 3) (66 entries); pi0 = 3 e_3;
    y1 = 2 e_3 + e_10 with q1 = 7."""
    a = {n: v for (c, n), v in arrays.items() if c == "slots"}
    m, MP, base, nnz = 65, 128, 7, 66
    # padded pointer tails: rp[i] = rp[m], cp[i] = cp[m] for m < i <= MP
    assert len(a["rp"]) == len(a["cp"]) == MP + 1
    assert a["rp"][m] == a["cp"][m] == base + nnz
    assert a["rp"][m:] == [base + nnz] * (MP + 1 - m) and a["cp"][m:] == [base + nnz] * (MP + 1 - m)
    assert a["rp"][:m] == [base + i for i in range(m)]                      # one entry per row before row 64
    assert a["cp"][:m] == [base + (i if i <= 3 else i + 1) for i in range(m)]   # column 3 holds two
    assert a["rc"] == list(range(64)) + [3, 64] and a["rv"] == [1.0] * 64 + [-4.0, 1.0]
    assert a["ci"] == [0, 1, 2, 3, 64] + list(range(4, 65))                 # rows ascending within column 3
    assert a["cv"] == [1.0] * 4 + [-4.0] + [1.0] * 61
    # hb: type 3 for the slack of the E row, 1 for the G row's, 2 for the L rows'; -1 past m
    hb = [4 * (2 + i) + 2 for i in range(m)]
    hb[0], hb[3], hb[64] = 4 * 2 + 3, 0, 4 * 66 + 1
    assert a["hb"] == hb + [-1] * (MP - m)
    # masks: columns 64 + j (j = 0, 1, 2: the slacks of rows 62, 63, 64) are bit 1 of word j;
    # columns 1 (y1) and 5 (the slack of row 3) are not basic
    basic = [1] * 64
    basic[0], basic[1], basic[2], basic[5] = 3, 2, 3, 0
    assert a["basic"] == basic
    for j in range(3):
        assert a["basic"][j] >> 1 & 1
    d0 = [0.0] * 128
    d0[1], d0[5] = 7.0 - 3.0 * 2.0, -3.0
    assert a["d0"] == d0
