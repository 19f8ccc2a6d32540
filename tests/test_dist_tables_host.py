"""The joint-distribution tables (sqlp_amd/csrc/dist_tables.h) on the CPU: a stand-alone program
that includes only that header (tests/native/dist_tables_check.cpp), built by the host compiler
with ASan + UBSan (`make sanitize_dist`) and run directly.  It compares the header's pick -- the
function the sampler kernels call -- with the literal DISCRETE walk at every running sum, its two
fp64 neighbours, 0 and 1 - 2^-53 of generated blocks, runs every validation error on arrays of
exactly the lengths the shapes give, and prints the tables of a permuted two-block layout."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# DistErr of dist_tables.h
CODES = {"ok": 0, "no_blocks": 0, "member_off_start": 2, "empty_block": 3, "nreal_zero": 4, "nreal_negative": 4, "too_large": 5,
         "member_low": 6, "member_high": 6, "member_kind": 7, "twice_in_one": 8, "in_two_blocks": 8, "in_no_block": 9,
         "kind3_without_blocks": 9, "prob_negative": 10, "prob_nan": 10, "prob_inf": 10, "value_nan": 11, "value_inf": 11}


@pytest.fixture(scope="module")
def lines():
    if shutil.which("make") is None or shutil.which("c++") is None:
        pytest.skip("make / c++ not available")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sqlp_amd", "csrc"), "sanitize_dist"])
    exe = os.path.join(ROOT, "sqlp_amd", "csrc", "build_san", "dist_tables_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    out = r.stdout.splitlines()
    assert out[-1] == "all ok"
    return out


def test_pick_equals_the_walk(lines):
    seen = {}
    for line in lines:
        if line.startswith("pick "):
            f = dict(re.findall(r"(\w+)=(\S+)", line))
            seen[(int(f["R"]), float(f["mass"]), int(f["zeros"]))] = f
            assert f["mismatches"] == "0", line
            assert int(f["probes"]) == 3 * int(f["R"]) + 2
    assert sorted(seen) == sorted((R, m, z) for R in (1, 2, 3, 7, 1000) for m in (1.0, 0.9, 0.0) for z in (0, 1, 2, 3))
    # the cases are what they say: zero-probability runs give ties in the running sums, the mass is the last sum
    for (R, m, z), f in seen.items():
        assert abs(float(f["last"]) - m) <= 1e-12
        if m == 0.0:
            assert int(f["ties"]) == R - 1
        elif z and R >= 7:
            assert int(f["ties"]) >= 2
        elif not z:
            assert int(f["ties"]) == 0


def test_every_validation_error_returns_its_code(lines):
    got = {}
    for line in lines:
        if line.startswith("error ") and "code=" in line:
            name = line.split()[1]
            f = dict(re.findall(r"(\w+)=(-?\d+)", line))
            got[name] = int(f["code"])
            assert f["kept"] == "1", line                 # the caller's tables are written on success only
    assert got == CODES
    assert "error null : kind=1 blocks=1 empty=0" in lines


def test_tables_of_a_permuted_layout(lines):
    """k = 7, block 0 = [4, 1, 6] with R = 2, block 1 = [0] with R = 3."""
    line, = [ln for ln in lines if ln.startswith("table ")]
    assert "rc=0 lead=0,4,2,3,4,5,4, blk=1,0,-1,-1,0,-1,0, col=0,1,0,0,0,0,2, blocks=(2,3,0,0)(3,1,2,6)" in line
    cum = [float(t) for t in re.search(r"cum=(\S+)", line).group(1).rstrip(",").split(",")]
    assert cum == [0.25, 0.25 + 0.5, 0.0, 0.0 + 0.1, (0.0 + 0.1) + 0.2]        # per block, sequential sums
    mad = [float(t) for t in re.search(r"mad=(\S+)", line).group(1).split(",")]
    # member 1 of block 0: values 11, 21 at p = 0.25, 0.5; block 1: values 1, 2, 3 at p = 0, 0.1, 0.2
    mu0 = (0.25 * 11 + 0.5 * 21) / 0.75
    mu1 = (0.1 * 2 + 0.2 * 3) / 0.3
    assert abs(mad[0] - (0.25 * abs(11 - mu0) + 0.5 * abs(21 - mu0)) / 0.75) <= 1e-12
    assert abs(mad[1] - (0.1 * abs(2 - mu1) + 0.2 * abs(3 - mu1)) / 0.3) <= 1e-12
