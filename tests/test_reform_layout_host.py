"""The layouts of a cut re-formed from stored picks (no GPU):
sqlp_amd/csrc/reform_layout.h in a stand-alone program (tests/native/reform_layout_check.cpp) built
by the host compiler with ASan + UBSan (`make sanitize_reform`) and run directly, every printed
number against a Python restatement of the formulas as boot_kernel.hip and risk.hip each wrote them
out before the header existed.  The bits of every re-formed cut depend on these layouts.

Sizes: scenario counts at the edges of one 64-scenario tile (63, 64, 65), of want = ceil(ntiles / 4)
(256, 257: 4 and 5 tiles; 2048, 2049: 32 and 33) and of the 512-shard cap (131072 = 2048 tiles = 512
shards of 4; 131073; 2^24, the largest epigraph); vertex counts at the 32-vertex floor (31, 32, 33)
and the 256-chunk cap (8192 = 256 x 32, 8193); offsets from the smallest call to 20 handles x 128
rows."""
import os
import shutil
import struct
import subprocess

import pytest

from tests import instances as I

ROOT = I.ROOT

NS = [1, 63, 64, 65, 256, 257, 2048, 2049, 131072, 131073, 2 ** 24]
NVS = [0, 1, 31, 32, 33, 8192, 8193, 100000]
OFFS = [(1, 0, 1, 0), (1, 1, 1, 1), (3, 33, 500, 70), (20, 64, 4096, 127)]


def _shards(n):
    ntiles = (n + 63) // 64
    want = min(512, (ntiles + 3) // 4)
    tpb = (ntiles + want - 1) // want
    return tpb, (ntiles + tpb - 1) // tpb


def _vchunks(nv):
    chunk = max(32, (nv + 255) // 256)
    return chunk, max(1, (nv + chunk - 1) // chunk)


def _offsets(H, M, nvs, k):
    B = M + 1
    o_wj = B
    o_hist = o_wj + H * B
    return B, o_wj, o_hist, o_hist + H * B * nvs, max(H * B * k, 1)


def _run_native(args):
    if shutil.which("make") is None or shutil.which("c++") is None:
        pytest.skip("make / c++ not available")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sqlp_amd", "csrc"), "sanitize_reform"])
    exe = os.path.join(ROOT, "sqlp_amd", "csrc", "build_san", "reform_layout_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return [line.split() for line in r.stdout.splitlines()]


def test_fixed_point_scale_is_two_to_the_58():
    (line,) = _run_native(["fix"])
    assert line[0] == "fix" and int(line[1], 16) == struct.unpack("<Q", struct.pack("<d", 2.0 ** 58))[0]
    assert 12 * 2 ** 58 < 2 ** 62          # twelve, the largest Poisson(1) count the thresholds give
    assert int(line[2]) == 512


def test_shard_layout_of_the_s_sums():
    out = _run_native(["shard"] + NS)
    assert len(out) == len(NS)
    for n, line in zip(NS, out):
        assert line[0] == "shard" and int(line[1]) == n
        tpb, nchunks = int(line[2]), int(line[3])
        assert (tpb, nchunks) == _shards(n), n
        ntiles = (n + 63) // 64
        assert 1 <= nchunks <= 512 and (nchunks - 1) * tpb < ntiles <= nchunks * tpb   # every shard holds a tile
    got = {int(l[1]): (int(l[2]), int(l[3])) for l in out}
    # by hand from the formulas: one tile; 5 tiles in 2 shards of 3; 33 tiles in 9 of 4; the cap
    assert got[1] == (1, 1) and got[257] == (3, 2) and got[2049] == (4, 9)
    assert got[131072] == (4, 512) and got[131073] == (5, 410) and got[2 ** 24] == (512, 512)


def test_vertex_chunks_of_the_g_partials():
    out = _run_native(["vchunk"] + NVS)
    assert len(out) == len(NVS)
    for nv, line in zip(NVS, out):
        assert line[0] == "vchunk" and int(line[1]) == nv
        chunk, nbc = int(line[2]), int(line[3])
        assert (chunk, nbc) == _vchunks(nv), nv
        assert chunk >= 32 and 1 <= nbc <= 256 and nbc * chunk >= nv
    got = {int(l[1]): (int(l[2]), int(l[3])) for l in out}
    assert got[0] == (32, 1) and got[33] == (32, 2) and got[8192] == (32, 256) and got[8193] == (33, 249)
    assert got[100000] == (391, 256)


def test_offsets_of_the_partial_buffers():
    out = _run_native(["off"] + [v for t in OFFS for v in t])
    assert len(out) == len(OFFS)
    for t, line in zip(OFFS, out):
        assert line[0] == "off" and tuple(int(v) for v in line[1:5]) == t
        assert tuple(int(v) for v in line[5:]) == _offsets(*t), t
    assert [int(v) for v in out[0][5:]] == [1, 1, 2, 3, 1]
    assert [int(v) for v in out[2][5:]] == [34, 34, 136, 51136, 7140]
