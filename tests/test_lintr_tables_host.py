"""The LINTR tables (sqlp_amd/csrc/lintr_tables.h) on the CPU: a stand-alone program that includes
only that header (tests/native/lintr_tables_check.cpp), built by the host compiler with ASan +
UBSan (`make sanitize_lintr`, which also runs it) and run directly.  It runs every validation
error on arrays of exactly the lengths the shapes give, the size guard from the shapes alone, and
prints the tables of a two-block layout with non-contiguous, descending members and rows of 0, 1
and q entries."""
import math
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# LintrErr of lintr_tables.h
CODES = {"ok": 0, "member_off_start": 2, "row_ptr_start": 2, "row_ptr_decreases": 2, "empty_block": 3, "no_latent": 4,
         "no_latent_first": 4, "too_large": 5, "member_low": 6, "member_high": 6, "member_kind": 7, "twice_in_one": 8,
         "in_two_blocks": 8, "in_no_block": 9, "kind4_without_blocks": 9, "column_low": 10, "column_high": 10,
         "column_high_second_block": 10, "column_repeated": 10, "column_descending": 10, "constant_nan": 11, "constant_inf": 11,
         "coef_nan": 12, "coef_inf": 12, "latent_kind": 13, "latent_kind_negative": 13, "latent_support_empty": 14,
         "latent_support_repeated": 14, "latent_prob_negative": 14, "latent_prob_nan": 14, "latent_variance_negative": 15,
         "latent_variance_nan": 15}


@pytest.fixture(scope="module")
def lines():
    if shutil.which("make") is None or shutil.which("c++") is None:
        pytest.skip("make / c++ not available")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sqlp_amd", "csrc"), "sanitize_lintr"], env=env)
    exe = os.path.join(ROOT, "sqlp_amd", "csrc", "build_san", "lintr_tables_check")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    out = r.stdout.splitlines()
    assert out[-1] == "all ok"
    return out


def _fields(line):
    return {k: [float(t) for t in v.rstrip(",").split(",")] if "," in v else v for k, v in re.findall(r"(\w+)=(\S+)", line)}


def test_every_validation_error_returns_its_code(lines):
    got = {}
    for line in lines:
        if line.startswith("error ") and "code=" in line:
            name = line.split()[1]
            f = dict(re.findall(r"(\w+)=(-?\d+)", line))
            got[name] = int(f["code"])
            assert f["kept"] == "1", line                 # the caller's tables are written on success only
    assert got == CODES
    assert "error null : constants=1 kind=1 val=1 empty=1" in lines
    assert "empty rc=0 M=0 Q=0 rptr=0," in lines


def test_tables_of_a_permuted_layout(lines):
    """k = 7; block 0 = members [5, 0, 3], q = 2, rows of 2, 1 and 0 entries; block 1 = members
    [6, 4], q = 3, rows of 3 and 1 entries."""
    t = _fields(next(ln for ln in lines if ln.startswith("table ")))
    assert t["rc"] == "0" and t["M"] == "5" and t["Q"] == "5"
    assert t["blk"] == [0, -1, -1, 0, 1, 0, 1] and t["row"] == [1, -1, -1, 2, 4, 0, 3]     # element -> (block, row)
    assert t["elem"] == [5, 0, 3, 6, 4] and t["c"] == [10, -2, 0.5, 1, 2]
    assert t["rptr"] == [0, 2, 3, 3, 6, 7]
    assert t["col"] == [0, 1, 1, 2, 3, 4, 3]               # block-local columns turned into global latent numbers
    assert t["h"] == [1.5, -0.5, 2, 1, 0, -3, 0.25]        # the explicit zero is kept
    la = _fields(next(ln for ln in lines if ln.startswith("latents ")))
    assert la["kind"] == [0, 2, 1, 1, 0] and la["off"] == [0, 3, 3, 3, 3, 5]
    assert la["word"] == [7, 8, 9, 10, 11]                 # k + l
    assert la["val"] == [-1, 0, 2, 1, 3] and la["prob"] == [0.5, 0.25, 0.25, 0.5, 0.5]     # supports sorted by value
    assert la["p0"] == [0, -1, 0, 5, 0] and la["p1"] == [0, 3, 1, 2, 0]                    # NORMAL: the standard deviation
    var = [0.5 * 1 + 0.25 * 0 + 0.25 * 4, 16.0 / 12.0, 1.0, 4.0, 1.0]                      # mean 0 for the first
    assert la["var"] == pytest.approx(var, rel=1e-15)
    m = _fields(next(ln for ln in lines if ln.startswith("members ")))
    want = [math.sqrt(2 / math.pi) * math.sqrt(v) for v in
            (1.5 ** 2 * var[0] + 0.5 ** 2 * var[1], 2.0 ** 2 * var[1], 0.0, 1.0 * var[2] + 0.0 * var[3] + 9.0 * var[4], 0.25 ** 2 * var[3])]
    assert m["mad"] == pytest.approx(want, rel=1e-14)
    # v = c, then v = v + (h * xi_l) in order, at xi = (2, 0.5, -1.25, 3, 1)
    assert m["value"] == [(10.0 + 1.5 * 2.0) + -0.5 * 0.5, -2.0 + 2.0 * 0.5, 0.5, ((1.0 + 1.0 * -1.25) + 0.0 * 3.0) + -3.0 * 1.0, 2.0 + 0.25 * 3.0]
