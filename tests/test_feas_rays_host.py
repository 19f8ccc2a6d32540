"""The arithmetic of feasibility rays (sqlp_amd/csrc/feas_rays.h) on the CPU: a stand-alone program
that includes only that header (tests/native/feas_rays_check.cpp), built by the host compiler with
ASan + UBSan and -ffp-contract=off (`make sanitize_feas`, which also runs it) and run directly.  It
prints the snapped and normalised ray, the key and a feasibility row for a table of cases; here
they are compared with numpy, bit for bit (the header pins the order of every sum)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def cases():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sqlp_amd", "csrc"), "sanitize_feas"], env=env)
    exe = os.path.join(ROOT, "sqlp_amd", "csrc", "build_san", "feas_rays_check")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    out, cur = {}, None
    for line in r.stdout.splitlines():
        tag, *rest = line.split()
        if tag == "case":
            cur = out.setdefault(rest[0], {"mv": int(rest[2]), "n1": int(rest[4])})
        elif tag in ("ok", "key"):
            cur[tag] = int(rest[0])
        elif tag == "alpha":
            cur[tag] = float.fromhex(rest[0])
        else:
            cur[tag] = np.array([float.fromhex(t) for t in rest])
    return out


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key_np(nrm):
    """Components rounded to 24 significant bits (sign, exponent, 23 mantissa bits; half up on the
    magnitude) next to their row, mixed and summed mod 2^64."""
    h = 0
    for i, v in enumerate(nrm):
        bits = int(np.array([0.0 if v == 0.0 else v]).view(np.uint64)[0])
        b = ((bits + (1 << 28)) & M64) >> 29
        h = (h + mix64(((i << 35) | b) & M64)) & M64
    return h


def snap_np(s, zero_rel=1e-12):
    s = s.copy()
    if np.isfinite(s).all():
        s[np.abs(s) <= zero_rel * (1.0 + np.abs(s).max())] = 0.0
    return s


def test_snap_normalise_and_key(cases):
    assert len(cases) == 12
    for name, c in cases.items():
        assert len(c["sigma"]) == c["mv"]
        s = snap_np(c["sigma"])
        np.testing.assert_array_equal(c["snapped"], s)
        good = bool(np.isfinite(s).all() and np.abs(s).max() > 0)
        assert c["ok"] == int(good), name
        if not good:
            assert "normalised" not in c and "key" not in c
            continue
        nrm = s / np.abs(s).max()
        np.testing.assert_array_equal(c["normalised"], nrm)
        assert not np.signbit(c["normalised"][c["normalised"] == 0]).any()         # zeros are +0
        assert np.abs(c["normalised"]).max() == 1.0
        assert c["key"] == key_np(nrm), name


def test_refused_rays(cases):
    assert [cases[n]["ok"] for n in ("zero", "nan", "inf")] == [0, 0, 0]


def test_key_properties(cases):
    assert cases["scaled"]["key"] == cases["signs"]["key"]                         # positive scaling
    np.testing.assert_array_equal(cases["scaled"]["normalised"], cases["signs"]["normalised"])
    assert cases["flipped"]["key"] != cases["signs"]["key"]                        # one component's sign
    assert cases["perturbed"]["key"] == cases["signs"]["key"]                      # below the 24-bit rounding
    assert not np.array_equal(cases["perturbed"]["normalised"], cases["signs"]["normalised"])
    t = cases["tiny"]
    assert t["snapped"][1] == 0.0 and t["snapped"][2] == 0.0 and t["snapped"][3] == 3e-12   # threshold 2e-12, inclusive
    assert cases["negzero"]["key"] == key_np(np.array([0.0, 1.0, 0.0]))


def test_row_in_the_stated_order(cases):
    """alpha = sum_i sigma_i rb_i and beta_j = -sum_i T_ij sigma_i, index order, every product and
    sum rounded on its own."""
    seen = 0
    for name, c in cases.items():
        if "alpha" not in c:
            continue
        seen += 1
        mv, n1 = c["mv"], c["n1"]
        sig, rb = c["normalised"], c["rb"]
        a = 0.0
        for i in range(mv):
            a = a + sig[i] * rb[i]
        assert c["alpha"] == a, name
        T = c["T"].reshape(mv, n1) if n1 else np.zeros((mv, 0))
        beta = np.zeros(n1)
        for j in range(n1):
            acc = 0.0
            for i in range(mv):
                acc = acc + T[i, j] * sig[i]
            beta[j] = -acc
        np.testing.assert_array_equal(c["beta"], beta)
    assert seen == 4
