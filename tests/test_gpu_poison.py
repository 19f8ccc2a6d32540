"""Results must not depend on device memory no kernel wrote (reference: a scenario's solve sees
only its own data, smps_routines.jl:50-62).  Two fresh child processes run the same storm
refresh + candidate lists + keyed solve/push + cut (tests/poison_child.py): one with every new
device allocation filled with 0xFF before it is returned (TWOSD_POISON=255, all three
allocation families: dalloc, grow-only arrays, cut workspace), one with allocations as they
come.  0xFF reads back as int -1 / NaN, so a read of unwritten memory either faults or changes
a result; every output is compared bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, tag, poison):
    env = dict(os.environ)
    env.pop("TWOSD_POISON", None)
    env.pop("TWOSD_POISON_FAMILY", None)
    if poison:
        env.update(TWOSD_POISON="255", TWOSD_POISON_FAMILY="7")
    out = tmp_path / f"{tag}.npz"
    r = subprocess.run([sys.executable, "-m", "tests.poison_child", str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{tag} child failed ({r.returncode}):\n{r.stderr[-3000:]}"
    # the hook announces itself once (devbuf.h poison_byte): the fill really was active
    assert ("TWOSD_POISON: new device allocations filled with 0xff" in r.stderr) == poison, r.stderr[-2000:]
    with np.load(out) as d:
        return {k: d[k] for k in d.files}


def test_results_independent_of_allocation_fill(tmp_path):
    clean = _run(tmp_path, "clean", False)
    poisoned = _run(tmp_path, "poison", True)
    assert set(clean) == set(poisoned)
    assert (clean["status"] == 0).all()
    assert clean["heads_a"].shape[0] > 1 and clean["heads_b"].shape[0] > 1
    for k in sorted(clean):
        a, b = clean[k], poisoned[k]
        assert a.shape == b.shape, k
        # bit for bit (NaN-safe: compare the bytes)
        assert a.tobytes() == b.tobytes(), f"{k} differs under the 0xFF allocation fill"
