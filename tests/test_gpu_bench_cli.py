"""bench.py's command line on a small storm workload (40,000 scenarios, |V| = 256), in fresh
child processes: a plain run times exactly --steps steps, prints one result line without the
legs that take runs of their own, and --dump-outputs writes the last timed step's outputs,
identical from run to run; --full brings the trajectory, the spot check, the push check and the
CPU baseline back and leaves the timed path's outputs unchanged."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--scenarios", "40000", "--vertices", "256",
         "--x-points", "0,4,12"]
FULL_LEGS = ("parity_spot_check", "push_check", "cpu_baseline")


def _bench(dump, *extra, **env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + ["--dump-outputs", str(dump)] +
                       list(extra), cwd=ROOT, env={**os.environ, **env}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"bench.py failed ({r.returncode}):\n{r.stderr[-3000:]}"
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    with os.scandir(dump) as it:
        arrs = {e.name[:-4]: np.load(e.path) for e in it if e.name.endswith(".npy")}
    return json.loads(lines[0]), arrs


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("plain"))


def test_plain_run_line_and_dump(plain):
    out, arrs = plain
    assert out["steps"] == 3 and len(out["steps_log"]["rows"]) == 3
    assert sum(p["steps"] for p in out["x_points"]) == 3
    assert out["unit"] == "subproblems/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(40000 / (out["ms_per_step"] * 1e-3), rel=1e-12)
    assert out["trajectory"] is None and not any(k in out for k in FULL_LEGS)
    assert set(arrs) == {"x", "cut_alpha", "cut_beta", "cut_weight_mark", "objective_sums", "new_vertices"}
    assert all(a.dtype == np.float64 for a in arrs.values())
    n1 = arrs["x"].shape[0]
    assert arrs["cut_beta"].shape == (1, n1) and arrs["objective_sums"].shape == (1, 2)
    # the last of the 3 timed steps ran at x point 2: the line reports the same cut and objective
    px = out["x_points"][2]
    assert arrs["cut_alpha"][0] == px["alpha"]
    assert arrs["objective_sums"][0, 0] / arrs["objective_sums"][0, 1] == px["incumbent_objective"]
    assert arrs["cut_weight_mark"][0] == 40000.0 and arrs["objective_sums"][0, 1] == 40000.0
    assert np.isfinite(arrs["cut_beta"]).all() and np.abs(arrs["cut_beta"]).max() > 0


def test_dump_is_identical_from_run_to_run(plain, tmp_path):
    _, again = _bench(tmp_path)
    assert set(again) == set(plain[1])
    for k, a in plain[1].items():
        assert a.tobytes() == again[k].tobytes(), k


def test_full_adds_the_other_legs(plain, tmp_path):
    # the CPU baseline takes 256 scenarios per thread and chunk, 6 legs of at least one chunk each:
    # 4 threads and a short budget keep it inside the 40,000 scenarios
    out, arrs = _bench(tmp_path, "--full", "--trajectory", "2", "--spot", "256", "--cpu-seconds", "0.2",
                       "--cpu-pool", "8", OMP_NUM_THREADS="4")
    assert out["steps"] == 3 and len(out["steps_log"]["rows"]) == 3
    assert out["trajectory"]["steps"] == 2
    assert len(out["parity_spot_check"]) == len(out["x_points"])
    assert all(s["lp_not_optimal"] == 0 and s["lp_obj_max_rel_err"] <= 1e-9 and s["cut_value_rel_err"] <= 1e-9
               for s in out["parity_spot_check"])
    assert out["push_check"]["identical"]
    assert out["cpu_baseline"]["value"] > 0
    for k, a in plain[1].items():
        assert a.tobytes() == arrs[k].tobytes(), k
