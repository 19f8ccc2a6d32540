"""The host side of the grouped bootstrap: how stopping.bootstrap_gap_test and
master.sd_run hand a sampling plan on, and the collective step of dist.reform_cuts_sharded on CPU
tensors (world_size 2, gloo).  No GPU: reform is a fake, the partials are made up."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from sqlp_amd import dist as sdist
from tests.test_boot_host import _fake_reform, _hand_cell
from tests.test_dist_moments_gloo import _free_port


def _recording(calls):
    inner = _fake_reform(0.01)

    def reform(epi, cuts, M, seed, index_offset=0, **kw):
        calls.append((epi, seed, index_offset, dict(kw)))
        return inner(epi, cuts, M, seed, index_offset)
    return reform


def _two_epigraph_cell():
    from sqlp_amd import twosd
    cell, epi, x0 = _hand_cell()
    epi.objective_weight = 0.5
    second = SimpleNamespace(objective_weight=0.5, lower_bound=0.0, total_scenario_weight=6.0,
                             cuts=[twosd.sdCut(390.0, np.array([-19.0, -14.0, -11.0, -12.0]), 6.0, picks=2)], incumbent_cut=None)
    cell.bind_epigraph(second)
    return cell, [epi, second]


def test_plan_reaches_reform_as_a_keyword_only_when_given():
    from sqlp_amd import stopping, twosd
    cell, epi, _ = _hand_cell()
    calls = []
    plain = stopping.bootstrap_gap_test(cell, M=4, seed=1, reform=_recording(calls))
    assert [c[3] for c in calls] == [{}]                       # no keyword at all: today's call
    plan = twosd.Sampling.antithetic()
    calls.clear()
    res = stopping.bootstrap_gap_test(cell, M=4, seed=1, reform=_recording(calls), sampling=plan)
    assert [c[3] for c in calls] == [{"sampling": plan}]
    np.testing.assert_array_equal(res.U, plain.U)              # the fake ignores the plan: the arithmetic is the same
    # the untouched fake of tests/test_boot_host.py (no sampling keyword) keeps working without a plan
    stopping.bootstrap_gap_test(cell, M=4, seed=1, reform=_fake_reform(0.01), sampling=None)


def test_a_list_of_plans_is_routed_by_epigraph_index():
    from sqlp_amd import stopping, twosd
    cell, epis = _two_epigraph_cell()
    lhs = twosd.Sampling.lhs(64)
    calls = []
    stopping.bootstrap_gap_test(cell, M=3, seed=7, reform=_recording(calls), sampling=[None, lhs], index_offsets=[0, 128])
    assert [(c[0], c[1], c[2], c[3]) for c in calls] == [(epis[0], 7, 0, {}), (epis[1], 8, 128, {"sampling": lhs})]
    calls.clear()
    stopping.bootstrap_gap_test(cell, M=3, seed=7, reform=_recording(calls), sampling=lhs)     # one plan: every epigraph
    assert [c[3] for c in calls] == [{"sampling": lhs}] * 2
    for bad in ([lhs], [lhs, None, None], []):
        with pytest.raises(ValueError, match=f"sampling lists {len(bad)} plans for 2 epigraphs"):
            stopping.bootstrap_gap_test(cell, M=3, reform=_recording(calls), sampling=bad)


def test_sd_run_hands_the_plan_to_the_default_stop_only(monkeypatch):
    from sqlp_amd import master, stopping, twosd
    seen = []
    monkeypatch.setattr(master, "sd_iteration", lambda cell, scen, **kw: None)
    monkeypatch.setattr(stopping, "bootstrap_gap_test", lambda cell, **kw: seen.append(kw) or SimpleNamespace(passed=True))
    plan = twosd.Sampling.antithetic()
    assert master.sd_run("cell", lambda it: [], 5, check_every=1, sampling=plan, stop_args={"M": 16})[0] == 1
    assert seen == [{"sampling": plan, "M": 16}]
    seen.clear()
    master.sd_run("cell", lambda it: [], 5, check_every=1)
    assert seen == [{}]                                         # without a plan the default stop is called as before
    mine = []
    master.sd_run("cell", lambda it: [], 5, check_every=1, sampling=plan, stop=lambda c: mine.append(c) or SimpleNamespace(passed=True))
    assert mine == ["cell"] and seen == [{}]                    # the caller's stop: stop(cell), no keyword


# ---------------------------------------------------------------- the collective step
BIG = 1 << 61      # per rank: two ranks reach 2^62, the bound of every uint64 sum of a re-formation


def _rank_partials(rank):
    """Recorded partials of one rank: int64 storage of the uint64 part, and the fp64 part."""
    rng = np.random.default_rng(100 + rank)
    u = rng.integers(0, BIG, size=257, dtype=np.int64)
    u[0], u[1], u[2] = BIG, BIG - 1 - rank, 0
    f = rng.normal(size=96) * 10.0 ** rng.integers(-6, 7, size=96)
    return u, f


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        u, f = _rank_partials(rank)
        tu, tf = sdist.allreduce_reform_partials(torch.from_numpy(u.copy()), torch.from_numpy(f.copy()))
        out[rank] = (tu.numpy().copy(), tf.numpy().copy())
    finally:
        dist.destroy_process_group()


def test_two_rank_reduction_of_reform_partials():
    port = _free_port()
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
        res = dict(out)
    (u0, f0), (u1, f1) = _rank_partials(0), _rank_partials(1)
    want_u = np.array([int(a) + int(b) for a, b in zip(u0, u1)], dtype=object)     # Python integers: exact
    assert int(want_u.max()) == 2 * BIG                         # 2^62: past fp64's 53 bits, inside int64
    for rank in (0, 1):
        gu, gf = res[rank]
        assert gu.dtype == np.int64 and [int(v) for v in gu] == list(want_u)
        np.testing.assert_array_equal(gf, f0 + f1)               # two terms: one rounding, any order
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])


def test_single_process_reduction_is_the_identity_and_checks_dtypes():
    u, f = _rank_partials(0)
    tu, tf = torch.from_numpy(u.copy()), torch.from_numpy(f.copy())
    ru, rf = sdist.allreduce_reform_partials(tu, tf)
    assert ru is tu and rf is tf
    np.testing.assert_array_equal(tu.numpy(), u)
    np.testing.assert_array_equal(tf.numpy(), f)
    with pytest.raises(TypeError):
        sdist.allreduce_reform_partials(tu.to(torch.int32), tf)
