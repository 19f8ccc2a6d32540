"""Writes tests/golden/sel_picks_r08.npz: the warm-start picks of storm batches under the flat and the
two-level pool selection (pool_select_kernel, pool_refine_kernel), which
tests/test_gpu_pool_select_paths.py compares a build against exactly, split and unsplit.  Run it on the
GPU at the commit whose picks the fixture pins (here: the commit before the level-2 kernel's launch
bound and tile order and the records' sentinel offset changed); a pull request that changes the
selection key on purpose runs it again and says so.
Usage: python tools/make_sel_golden.py [out.npz]

The set-up is that of test_pool_selection_split_equals_one_chunk (tests/test_gpu_lp.py): storm at
x_EV with distributions set, pool_refresh(8192 training scenarios, 1024 bases),
pool_build_candidates(128, 160), evaluation scenarios drawn on the device with a fixed seed.  Cases:
  flat        N = 129 and 4096, before the candidate lists exist (least key over the whole pool)
  two-level   N = 1, 127, 128, 129 and 4096 (one lane, a tile short of one scenario, a full tile,
              a second tile of one scenario, 32 tiles)
each at x_EV and at a second x away from it (x_EV scaled per component; the fixture holds it).  Every
LP of every case ends optimal.  Only picks are stored.
The set-up and the per-case run live here and are imported by the test, so the fixture and the test
cannot drift apart."""
import contextlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_lp_paths_golden as G  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "sel_picks_r08.npz")
TRAIN, TRAIN_SEED, POOL = 8192, 41, 1024
LEVEL1, NCAND = 128, 160
N_EVAL, EVAL_SEED = 4096, 42
FLAT_N = (129, 4096)
TWO_N = (1, 127, 128, 129, 4096)
X2_SCALES = (0.2, 0.05, 0.01)   # the second x: the first of these for which every LP ends optimal
KNOBS = ("TWOSD_SEL_NOSPLIT",)


@contextlib.contextmanager
def launch_env(**env):
    """The selection's launch knobs (read by the library at every launch) set for the block, the others unset."""
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in env.items():
            assert k in KNOBS, k
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def second_x(x, scale):
    """x_EV with every component scaled by 1 + scale * sin(1 + i) (stays non-negative)."""
    return x * (1.0 + scale * np.sin(1.0 + np.arange(len(x))))


def picks_of(ctx, x, epi, N):
    """(picks, all optimal) of the first N evaluation scenarios at x."""
    from sqlp_amd import twosd
    _, _, _, st = twosd.solve_batch(epi, x, 0, N, want_pi=False)
    return np.asarray(ctx.last_pool_picks(N)).copy(), bool((st == 0).all())


def build_flat():
    """(ctx, x_EV, evaluation epigraph, training epigraph) with the refreshed pool and no candidate
    lists yet: the selection is flat."""
    from sqlp_amd import twosd
    ctx, x, sto = G.new_ctx("storm")
    ctx.set_distributions(sto)
    tr = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(tr, TRAIN, TRAIN_SEED)
    assert ctx.pool_refresh(tr, x, 0, TRAIN, POOL) > LEVEL1
    ev = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(ev, N_EVAL, EVAL_SEED)
    return ctx, x, ev, tr


def add_candidates(ctx, x, tr):
    """From here on the selection is two-level."""
    ctx.pool_build_candidates(tr, x, 0, TRAIN, LEVEL1, NCAND)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    data = {}
    with launch_env():
        ctx, x, ev, tr = build_flat()
        x2 = None
        for scale in X2_SCALES:
            cand = second_x(x, scale)
            _, ok = picks_of(ctx, cand, ev, N_EVAL)
            print(json.dumps({"second_x_scale": scale, "all_optimal": ok}), flush=True)
            if ok:
                x2 = cand
                break
        assert x2 is not None, "no second x at which every LP ends optimal"
        data["x2"] = x2
        points = (("ev", x), ("x2", x2))
        for tag, xp in points:
            for N in FLAT_N:
                p, ok = picks_of(ctx, xp, ev, N)
                assert ok
                data[f"flat/{tag}/{N}"] = p
        add_candidates(ctx, x, tr)
        for tag, xp in points:
            for N in TWO_N:
                p, ok = picks_of(ctx, xp, ev, N)
                assert ok
                data[f"two/{tag}/{N}"] = p
    for tag, _ in points:
        f, t = data[f"flat/{tag}/{N_EVAL}"], data[f"two/{tag}/{N_EVAL}"]
        assert (t >= LEVEL1).any(), "level 2 replaced no pick"
        print(json.dumps({"x": tag, "flat_distinct": int(len(np.unique(f))), "two_distinct": int(len(np.unique(t))),
                          "two_from_level2": int((t >= LEVEL1).sum()), "two_equals_flat": int((t == f).sum())}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **data)
    print(f"wrote {out_path}: {os.path.getsize(out_path)} bytes", flush=True)


if __name__ == "__main__":
    main()
