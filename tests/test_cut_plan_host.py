"""The cut's launch plan (sqlp_amd/csrc/cut_plan.h) on the CPU: a stand-alone program that includes
only that header (tests/native/cut_plan_check.cpp), built by the host compiler with ASan + UBSan
(`make sanitize_plan`) and run directly, prints the plan of a table of shapes; the values below were
computed from the expressions the driver held before the plan was a function of its own
(kCutTile2 = 128, kVT2 = 32, kCandC = 16, default knobs unless stated, fix_per_cu = 3)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, nv, k, CUs, bpc, knob) -> full, S, nunits, nblocks, fx_gs, fix_blocks, ntail, merge_blocks, resc_blocks, slots;
#                               slot_fix, slot_merge, slot_rescan; cand_need, tcand_need
ROW_1000 = ((0, 2, 16, 16, 16, 16, 1000, 250, 4, 1144), (64, 128, 1128), (0, 131072))
TABLE = {
    (1, 1, 0, 256, 3, "default"): ((1, 1, 1, 1, 16, 1, 0, 0, 1, 12), (4, 8, 8), (8192, 0)),
    (300, 40, 3, 256, 3, "default"): ((3, 1, 3, 3, 16, 5, 0, 0, 2, 40), (12, 32, 32), (24576, 0)),
    (1000, 256, 5, 256, 3, "default"): ROW_1000,
    (1000, 257, 5, 256, 3, "default"): ROW_1000,
    (100000, 1000, 86, 256, 3, "default"): ((768, 8, 880, 768, 32, 768, 1696, 256, 256, 8192), (3072, 6144, 7168), (6291456, 917504)),
    (100000, 1000, 86, 256, 2, "default"): ((512, 7, 2402, 512, 32, 768, 34464, 256, 256, 7168), (2048, 5120, 6144), (4194304, 15482880)),
    (1000000, 5000, 117, 256, 3, "default"): ((7680, 23, 10739, 768, 64, 768, 16960, 256, 256, 8192), (3072, 6144, 7168),
                                              (62914560, 25059328)),
    (1000000, 5000, 117, 256, 3, "tail=0"): ((7813, 1, 7813, 768, 64, 768, 0, 0, 256, 7168), (3072, 6144, 6144), (64004096, 0)),
    (98304, 2048, 8, 256, 3, "default"): ((768, 1, 768, 768, 32, 768, 0, 0, 256, 7168), (3072, 6144, 6144), (6291456, 0)),
    (98305, 2048, 8, 256, 3, "default"): ((768, 16, 784, 768, 32, 768, 1, 1, 256, 7172), (3072, 6144, 6148), (6291456, 131072)),
    (125000, 260, 8, 256, 3, "default"): ((768, 2, 1186, 768, 32, 768, 26696, 256, 256, 8192), (3072, 6144, 7168), (6291456, 3424256)),
}
MAIN = ("full", "S", "nunits", "nblocks", "fx_gs", "fix_blocks", "ntail", "merge_blocks", "resc_blocks", "slots")
BASES = ("slot_fix", "slot_merge", "slot_rescan")
LOGS = ("cand_need", "tcand_need")
KBS = (1, 2, 4, 6, 8, 12, 16, 22, 24, 30, 32)


@pytest.fixture(scope="module")
def output():
    if shutil.which("make") is None or shutil.which("c++") is None:
        pytest.skip("make / c++ not available")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "sqlp_amd", "csrc"), "sanitize_plan"])
    exe = os.path.join(ROOT, "sqlp_amd", "csrc", "build_san", "cut_plan_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for name in list(env):
        if name.startswith("TWOSD_"):
            del env[name]
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    plans, passes = {}, {}
    for line in r.stdout.splitlines():
        head, _, body = line.partition(" : ")
        w = head.split()
        if w[0] == "plan":
            key = tuple(int(t) for t in w[1:6]) + (w[6],)
            plans[key] = body if body.startswith("refused") else {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)", body)}
        else:
            f = {a: int(b) for a, b in re.findall(r"(\w+)=(-?\d+)", line)}
            passes[f["k"]] = f
    return plans, passes


def test_table_rows(output):
    plans, _ = output
    for key, (main, bases, logs) in TABLE.items():
        p = plans[key]
        assert tuple(p[f] for f in MAIN) == main, (key, p)
        assert tuple(p[f] for f in BASES) == bases, (key, p)
        assert tuple(p[f] for f in LOGS) == logs, (key, p)
    assert plans[(1000, 256, 5, 256, 3, "default")]["hist_lds"] == 1
    assert plans[(1000, 257, 5, 256, 3, "default")]["hist_lds"] == 0


def test_slot_ranges_and_units(output):
    plans, _ = output
    for key in TABLE:
        p = plans[key]
        # four per block, disjoint, in the order argmax, fixup, merge, rescan, and nothing else
        edges = [0, p["slot_fix"], p["slot_merge"], p["slot_rescan"], p["slots"]]
        sizes = [4 * p[b] for b in ("nblocks", "fix_blocks", "merge_blocks", "resc_blocks")]
        assert [b - a for a, b in zip(edges, edges[1:])] == sizes, (key, p)
        assert sum(sizes) == p["slots"]
        assert p["nunits"] == p["full"] + (p["ntiles"] - p["full"]) * p["S"], (key, p)
        if p["S"] > 1:
            assert p["S"] <= min(64, p["nchunks"] // 4), (key, p)


def test_refusals(output):
    plans, _ = output
    big = plans[(67108864, 32, 1, 256, 3, "default")]
    assert big.startswith("refused log") and "cand_need=4294967296 " in big    # one past UINT32_MAX
    assert plans[(300, 40, 3, 256, 3, "log_max=4096")].startswith("refused log")
    assert plans[(1000, 64, 128, 256, 3, "default")] == "refused envelope"
    assert plans[(1000, 64, 127, 256, 3, "default")]["KB"] == 32


def test_passes(output):
    plans, passes = output
    assert sorted(passes) == list(range(128))
    for k, f in passes.items():
        k4 = (max(k, 1) + 3) & ~3
        assert f["k4"] == k4
        assert f["KB"] == min(kb for kb in KBS if 4 * kb >= k + 1)      # the element rows and the base row
        assert f["KB32"] == min(kb for kb in KBS if 4 * kb >= k4)       # the element rows only
        assert f["KS8"] == (1 if k4 <= 64 else 2)
    d, no_i8, no_f32 = (plans[(300, 40, 3, 256, 3, n)] for n in ("default", "i8=0", "f32=0"))
    assert (d["want32"], d["wanti8"]) == (1, 1) and (no_i8["want32"], no_i8["wanti8"]) == (1, 0)
    assert (no_f32["want32"], no_f32["wanti8"], no_f32["rows32"]) == (0, 0, 0)
    assert (d["vcap32"], d["rows"], d["rows32"]) == (64, 4, 8)
