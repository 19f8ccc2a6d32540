"""On-device scenario sampler (rand(rng, sto) smps_sto.jl:117-149) against
the C oracle (oracle/sampler.c, pinned by the Philox4x32-10 known answers): DISCRETE and
UNIFORM elements bit-exact, NORMAL within 1e-12 (device log/cos vs glibc)."""
import numpy as np
import pytest

from tests import instances as I

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["storm", "ssn", "transship", "lands"])
def test_device_sampler_matches_oracle(name):
    from oracle import cpu
    from sqlp_amd import twosd
    inst = I.load(name)
    ctx = twosd.SDContext(inst["sp2"], inst["sto"])
    ctx.set_distributions(inst["sto"])
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    N, seed = 20000, 0x5EED1234ABCDEF
    twosd.add_sampled_scenarios(epi, N, seed, first_index=7)
    assert epi.num_scenarios == N and epi.total_scenario_weight == N
    got = twosd.get_scenarios(epi)
    ref = cpu.sample_deltas(inst["sto"], ctx.positions, ctx.template_values, N, seed, 7) + ctx.template_values
    kinds = np.array([inst["sto"].indep[p][0] for p in ctx.positions])
    exact = kinds != "NORMAL"
    np.testing.assert_array_equal(got[:, exact], ref[:, exact])
    if (~exact).any():
        np.testing.assert_allclose(got[:, ~exact], ref[:, ~exact], rtol=1e-12, atol=1e-12)


def test_device_sampler_sharding_and_solve():
    """Shards (first_index) reproduce one stream; sampled scenarios solve like host ones."""
    from sqlp_amd import twosd
    inst = I.load("storm")
    ctx = twosd.SDContext(inst["sp2"], inst["sto"])
    ctx.set_distributions(inst["sto"])
    x = I.x_ev("storm")
    from sqlp_amd import smps
    ctx.compute_basis(x, smps.mean_values(inst["sto"]))
    a = twosd.sdEpigraph(ctx, 1.0, 0.0)
    b = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(a, 4096, 99)
    twosd.add_sampled_scenarios(b, 1000, 99, first_index=0)
    twosd.add_sampled_scenarios(b, 3096, 99, first_index=1000)
    np.testing.assert_array_equal(twosd.get_scenarios(a), twosd.get_scenarios(b))
    obj_a, _, _, st = twosd.solve_batch(a, x, want_pi=False)
    obj_h, _, _, st_h = ctx.solve_values(x, twosd.get_scenarios(a), want_pi=False)
    assert (st == 0).all() and (st_h == 0).all()
    np.testing.assert_allclose(obj_a, obj_h, rtol=1e-12)


@pytest.mark.parametrize("name", ["lands", "storm"])
def test_evaluate_sampled(name):
    """evaluate(sp1, sp2, sto, x; N) on device-drawn scenarios == the same scenarios
    (oracle stream) solved through solve_values and summed in order (smps_routines.jl:79)."""
    from oracle import cpu
    from sqlp_amd import smps, twosd
    inst = I.load(name)
    ctx = twosd.SDContext(inst["sp2"], inst["sto"])
    ctx.set_distributions(inst["sto"])
    x = I.x_ev(name)
    ctx.compute_basis(x, smps.mean_values(inst["sto"]))
    c1 = np.ones(len(x))
    N, seed = 30000, 4242
    val = twosd.evaluate_sampled(ctx, c1, x, N, seed)
    vals = cpu.sample_deltas(inst["sto"], ctx.positions, ctx.template_values, N, seed) + ctx.template_values
    ref = twosd.evaluate(ctx, c1, x, vals)
    assert abs(val - ref) <= 1e-10 * (1 + abs(ref))
    # two shards of the stream add up to the whole
    h = N // 3
    s_a = twosd.evaluate_sampled(ctx, np.zeros(len(x)), x, N, seed, 0, h)
    s_b = twosd.evaluate_sampled(ctx, np.zeros(len(x)), x, N, seed, h, N - h)
    assert abs(float(np.dot(c1, x)) + s_a + s_b - val) <= 1e-10 * (1 + abs(val))


def _mixed_sto(S):
    """The three kinds mixed over the k random rhs rows of a generated template (the construction
    of tests/test_oracle_kat.py::test_sampler_oracle_distributions), with the DISCRETE edges: a
    one-point support, and probabilities that sum to 0.9, so that a tenth of the draws run the
    cumulative scan to its `i < n - 1` stop."""
    from sqlp_amd.smps import spSmpsPosition, spStoType
    dists = [("DISCRETE", [1.0, 4.0, 2.0], [0.3, 0.3, 0.3]), ("NORMAL", 10.0, 4.0), ("UNIFORM", -1.0, 3.0),
             ("DISCRETE", [2.5], [1.0]), ("DISCRETE", [7.0, 3.0, 5.0], [0.3, 0.3, 0.4]), ("UNIFORM", 100.0, 100.5),
             ("NORMAL", -3.0, 0.25), ("DISCRETE", [-1.0, 1.0], [0.5, 0.5])]
    sto = spStoType("synthetic", {})
    for e, (col, row) in enumerate(S.positions):
        sto.indep[spSmpsPosition(col, row)] = dists[e % len(dists)]
    return sto


@pytest.mark.parametrize("tid", ["c", "e"])
def test_sampler_mixed_kinds_and_counter_carry(tid):
    """UNIFORM elements (no shipped .sto has one), the DISCRETE edges, a seed with a nonzero high
    word, and scenario indices that carry into the high counter word inside the batch: N k is no
    multiple of the 256-thread block, so the last block is ragged.  Two shards that split at the
    carry reproduce the single draw."""
    from oracle import cpu
    from sqlp_amd import twosd
    from tests import synth_cases as SC
    S = SC.template(tid)
    sto = _mixed_sto(S)
    ctx = twosd.SDContext(S.sp2, sto)
    ctx.set_distributions(sto)
    N, seed, first = 1000, 0x9E3779B97F4A7C15, 2 ** 32 - 300
    assert (N * S.k) % 256 and seed >> 32
    epi = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(epi, N, seed, first_index=first)
    got = twosd.get_scenarios(epi)
    ref = cpu.sample_deltas(sto, ctx.positions, ctx.template_values, N, seed, first) + ctx.template_values
    kinds = np.array([sto.indep[p][0] for p in ctx.positions])
    assert set(kinds) == {"DISCRETE", "NORMAL", "UNIFORM"}
    exact = kinds != "NORMAL"
    np.testing.assert_array_equal(got[:, exact], ref[:, exact])
    np.testing.assert_allclose(got[:, ~exact], ref[:, ~exact], rtol=1e-12, atol=1e-12)
    # the reference itself has what the case is about: the high counter word matters, the short
    # DISCRETE element reaches its last value past its probability mass, UNIFORM stays in range
    low = cpu.sample_deltas(sto, ctx.positions, ctx.template_values, N, seed, first - 2 ** 32) + ctx.template_values
    assert (low[:300] != ref[:300]).any() and (low[300:] != ref[300:]).any()
    assert np.allclose(ref[:, 3], 2.5) and 0.3 < np.isclose(ref[:, 0], 4.0).mean() < 0.5
    assert ref[:, 2].min() >= -1.0 - 1e-12 and ref[:, 2].max() < 3.0 and len(np.unique(ref[:, 2])) > N - 5
    two = twosd.sdEpigraph(ctx, 1.0, 0.0)
    twosd.add_sampled_scenarios(two, 300, seed, first_index=first)
    twosd.add_sampled_scenarios(two, N - 300, seed, first_index=2 ** 32)
    np.testing.assert_array_equal(twosd.get_scenarios(two), got)
