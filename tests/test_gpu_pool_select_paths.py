"""The warm-start picks of the flat and the two-level pool selection, pinned exactly against
tests/golden/sel_picks_r08.npz (tools/make_sel_golden.py, which builds the set-up for the fixture
and for this test; the fixture was recorded on the build before the level-2 kernel ran two blocks
per CU with tile = block and before row-start records carried the sentinel offset).

No scenario's key depends on which block evaluates its tile or next to which other tile, and the
chunked merge keeps the in-block rules, so the picks are the fixture's with one chunk per tile
(TWOSD_SEL_NOSPLIT) and with the split the batch size asks for.  Batch sizes: one lane, a tile short
of one scenario, a full tile, a second tile of one scenario, 32 tiles; at x_EV and at a second x."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_sel_golden as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(S.FIXTURE)


@pytest.fixture(scope="module")
def flat():
    with S.launch_env():
        ctx, x, ev, _ = S.build_flat()
    return ctx, x, ev


@pytest.fixture(scope="module")
def two():
    with S.launch_env():
        ctx, x, ev, tr = S.build_flat()
        S.add_candidates(ctx, x, tr)
    return ctx, x, ev


def point(golden, x, tag):
    return x if tag == "ev" else golden["x2"]


def test_fixture_holds_both_levels(golden):
    for tag in ("ev", "x2"):
        f, t = golden[f"flat/{tag}/{S.N_EVAL}"], golden[f"two/{tag}/{S.N_EVAL}"]
        assert len(f) == len(t) == S.N_EVAL
        assert (t >= S.LEVEL1).any() and (t < S.LEVEL1).any()     # level 2 replaced some picks, kept others
        assert len(np.unique(f)) > S.LEVEL1
        for N in S.TWO_N:                                          # a prefix of the batch is the batch's prefix
            np.testing.assert_array_equal(golden[f"two/{tag}/{N}"], t[:N])
    assert not np.array_equal(golden["x2"], S.G.load_instance("storm")[2])


@pytest.mark.parametrize("tag", ["ev", "x2"])
@pytest.mark.parametrize("N", S.FLAT_N)
def test_flat_picks(N, tag, flat, golden):
    ctx, x, ev = flat
    with S.launch_env():
        p, ok = S.picks_of(ctx, point(golden, x, tag), ev, N)
    assert ok
    np.testing.assert_array_equal(p, golden[f"flat/{tag}/{N}"])


@pytest.mark.parametrize("tag", ["ev", "x2"])
@pytest.mark.parametrize("N", S.TWO_N)
def test_two_level_picks(N, tag, two, golden):
    ctx, x, ev = two
    with S.launch_env():
        p, ok = S.picks_of(ctx, point(golden, x, tag), ev, N)
    assert ok
    np.testing.assert_array_equal(p, golden[f"two/{tag}/{N}"])


@pytest.mark.parametrize("tag", ["ev", "x2"])
@pytest.mark.parametrize("N", S.TWO_N)
def test_two_level_picks_one_chunk(N, tag, two, golden):
    ctx, x, ev = two
    with S.launch_env(TWOSD_SEL_NOSPLIT=1):
        p, ok = S.picks_of(ctx, point(golden, x, tag), ev, N)
    assert ok
    np.testing.assert_array_equal(p, golden[f"two/{tag}/{N}"])


@pytest.mark.parametrize("N", S.FLAT_N)
def test_flat_picks_one_chunk(N, flat, golden):
    ctx, x, ev = flat
    with S.launch_env(TWOSD_SEL_NOSPLIT=1):
        p, ok = S.picks_of(ctx, x, ev, N)
    assert ok
    np.testing.assert_array_equal(p, golden[f"flat/ev/{N}"])
