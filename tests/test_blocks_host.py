"""Joint discrete distributions on the host: the numpy restatement
tests/blocks_ref.py against tests/vr_ref.py, the loader's BLOCKS DISCRETE / SCENARIOS DISCRETE
sections with their errors, the layout and the host helpers (mean_values, sample_values,
joint_support), and the library's new symbol."""
import ctypes
import os

import numpy as np
import pytest

from sqlp_amd import smps
from sqlp_amd.smps import spSmpsPosition as Pos
from tests import blocks_ref as B
from tests import vr_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data", "smps")

LANDS3_P = [0.15, 0.25, 0.15, 0.20, 0.15, 0.10]
LANDS3_V = [[3, 3, 2], [5, 3, 2], [7, 3, 2], [5, 2, 3], [4, 4, 1], [6, 1, 4]]
LANDS3_POS = [Pos("RHS", "S2C5"), Pos("RHS", "S2C6"), Pos("RHS", "S2C7")]


# ---- the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["iid", "antithetic", ("lhs", 5)])
def test_one_member_ascending_block_is_the_indep_stream(plan):
    """Element 2 of k = 4 as a one-member block with ascending values (probabilities summing to 0.9,
    one of them 0): bit for bit the vr_ref stream of the same element as INDEP DISCRETE, and the
    other elements are untouched."""
    disc = ("DISCRETE", [-1.0, 0.5, 2.0, 7.0], [0.2, 0.0, 0.3, 0.4])
    dists = [("UNIFORM", -1.0, 3.0), ("DISCRETE", [4.0, 1.0], [0.5, 0.5]), disc, ("NORMAL", 10.0, 4.0)]
    blocked = list(dists)
    blocked[2] = ("BLOCK",)
    blocks = [([2], disc[2], np.array(disc[1])[:, None])]
    N, seed, first = 1000, 0x9E3779B97F4A7C15, 2 ** 32 - 300
    if plan == ("lhs", 5):
        first -= first % 5                          # on the group boundary below; still carries inside the batch
    want = {"iid": lambda: V.iid(dists, N, seed, first), "antithetic": lambda: V.antithetic(dists, N, seed, first)}.get(
        plan, lambda: V.lhs(dists, 5, N, seed, first))()
    got = B.draw(plan, blocked, blocks, N, seed, first)
    np.testing.assert_array_equal(got, want)
    assert len(np.unique(got[:, 2])) == 3 and (got[:, 2] == 7.0).mean() > 0.4   # 0.4 plus the missing tenth


def test_block_members_share_the_leads_draw():
    """Members listed [3, 0, 2]: all three columns follow the walk at the uniform of element word 3."""
    probs = [0.0, 0.5, 0.0, 0.25, 0.25, 0.0]
    values = np.arange(18, dtype=np.float64).reshape(6, 3)
    dists = [("BLOCK",), ("UNIFORM", 0.0, 1.0), ("BLOCK",), ("BLOCK",)]
    N, seed = 4000, 99
    out = B.iid(dists, [([3, 0, 2], probs, values)], N, seed, 5)
    u1, _ = V.uniforms(seed, 5 + np.arange(N, dtype=np.uint64), 4)
    i = B.walk(probs, u1[:, 3])
    assert set(np.unique(i)) == {1, 3, 4}                                   # zero-probability realisations never
    np.testing.assert_array_equal(out[:, [3, 0, 2]], values[i])
    np.testing.assert_array_equal(out[:, 1], u1[:, 1])
    # the walk against a plain loop, at the edges: u on a running sum, past the mass, mass 0
    for p, u in [(probs, 0.5), (probs, 0.4999999), (probs, 0.75), (probs, 1.0), ([0.3, 0.3, 0.3], 0.95), ([0.0, 0.0], 0.0)]:
        j, cp = 0, p[0]
        while cp <= u and j < len(p) - 1:
            j += 1
            cp = cp + p[j]
        assert B.walk(p, np.array([u]))[0] == j


# ---- the loader -------------------------------------------------------------------------------------
def _write(tmp_path, text, name="t.sto"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def test_lands3b_and_lands3s_load_to_the_same_tables():
    tables = []
    for name in ("lands3b", "lands3s"):
        cor, tim, sto = smps.load_smps(os.path.join(DATA, name))
        assert sto.indep == {} and len(sto.blocks) == 1
        b = sto.blocks[0]
        assert b.period == "PERIOD2" and b.positions == LANDS3_POS
        tables.append((b.positions, b.probs, np.asarray(b.values)))
        sp2 = smps.get_smps_stage_template(cor, tim, 2)
        pos, rows, cols = smps.scenario_positions(sp2, sto)
        assert pos == LANDS3_POS and rows.tolist() == [4, 5, 6] and cols.tolist() == [-1, -1, -1]
    assert tables[0][1] == tables[1][1] == LANDS3_P
    np.testing.assert_array_equal(tables[0][2], np.array(LANDS3_V, dtype=np.float64))
    np.testing.assert_array_equal(tables[1][2], tables[0][2])
    assert smps.load_smps(os.path.join(DATA, "lands3b"))[2].blocks[0].name == "BLOCK1"
    # the core and time files are lands' with the name changed
    for ext in ("cor", "tim"):
        a = open(os.path.join(DATA, "lands", f"lands.{ext}")).read()
        for name, tag in (("lands3b", "LandS3b"), ("lands3s", "LandS3s")):
            b = open(os.path.join(DATA, name, f"{name}.{ext}")).read()
            assert b == a.replace("LandS", tag, 1)


@pytest.mark.parametrize("name", ["lands", "newsvendor", "transship", "ssn", "storm"])
def test_shipped_instances_have_no_blocks(name):
    from oracle import smps_ref
    d = os.path.join(DATA, name)
    cor, tim, sto = smps.load_smps(d, name)
    assert sto.blocks == []
    _, _, osto = smps_ref.load_instance(d, name)
    assert list(sto.indep.keys()) == [Pos(*p) for p in osto.indep.keys()]
    for p, od in osto.indep.items():
        mine = sto.indep[Pos(*p)]
        assert mine[0] == od[0] and list(np.ravel(mine[1])) == list(np.ravel(od[1])) and list(np.ravel(mine[2])) == list(np.ravel(od[2]))
    assert smps.sto_positions(sto) == list(sto.indep.keys())
    assert smps.read_sto(os.path.join(d, name + ".sto")).indep == sto.indep       # without the core file too


MIXED = """STOCH         mixed
INDEP         DISCRETE
    RHS       R1        1.0   0.5
    RHS       R1        2.0   0.5
BLOCKS        DISCRETE
 BL B1        P2        0.5
    X1        R3        1.0
    RHS       R2        2.0
 BL B2        P2        1.0
    RHS       R5        9.0
 BL B1        P2        0.25
    RHS       R2        4.0
INDEP         NORMAL
    RHS       R4        0.0   1.0
BLOCKS        DISCRETE
 BL B1        P2        0.25
    X1        R3        -1.0
ENDATA
"""


def test_sections_in_any_order_and_the_layout(tmp_path):
    sto = smps.read_sto(_write(tmp_path, MIXED))
    assert list(sto.indep.keys()) == [Pos("RHS", "R1"), Pos("RHS", "R4")]
    assert [b.name for b in sto.blocks] == ["B1", "B2"]
    b1, b2 = sto.blocks
    assert b1.positions == [Pos("X1", "R3"), Pos("RHS", "R2")] and b1.probs == [0.5, 0.25, 0.25]
    assert b1.values == [[1.0, 2.0], [1.0, 4.0], [-1.0, 2.0]]                 # omitted members: the first realisation's
    assert b2.positions == [Pos("RHS", "R5")] and b2.values == [[9.0]] and b2.probs == [1.0]
    # the layout: the INDEP keys, then each block's members in file order
    want = [Pos("RHS", "R1"), Pos("RHS", "R4"), Pos("X1", "R3"), Pos("RHS", "R2"), Pos("RHS", "R5")]
    assert smps.sto_positions(sto) == want
    from types import SimpleNamespace
    sp2 = SimpleNamespace(stage_constraints=["R1", "R2", "R3", "R4", "R5"], last_stage_vars=["X0", "X1"])
    pos, rows, cols = smps.scenario_positions(sp2, sto)
    assert pos == want and rows.tolist() == [0, 3, 2, 1, 4] and cols.tolist() == [-1, -1, 1, -1, -1]
    np.testing.assert_allclose(smps.mean_values(sto), [1.5, 0.0, 0.5, 2.5, 9.0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(smps.mean_values(sto, [Pos("RHS", "R2"), Pos("RHS", "R1")]), [2.5, 1.5], rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="NORMAL"):
        smps.joint_support(sto)


HEAD = "STOCH         t\n"
BL = "BLOCKS        DISCRETE\n"
ERRORS = {
    "absent from its first realisation": BL + " BL B1 P2 0.5\n    RHS R1 1.0\n BL B1 P2 0.5\n    RHS R2 1.0\n",
    "period 'P3' after 'P2'": BL + " BL B1 P2 0.5\n    RHS R1 1.0\n BL B1 P3 0.5\n    RHS R1 2.0\n",
    "is in blocks B1 and B2": BL + " BL B1 P2 1.0\n    RHS R1 1.0\n BL B2 P2 1.0\n    RHS R1 2.0\n",
    "is in block B1 and in INDEP": BL + " BL B1 P2 1.0\n    RHS R1 1.0\nINDEP DISCRETE\n    RHS R1 1.0 1.0\n",
    "in block B1 and in INDEP": "INDEP DISCRETE\n    RHS R1 1.0 1.0\n" + BL + " BL B1 P2 1.0\n    RHS R1 1.0\n",
    "probability 'half' is not a number": BL + " BL B1 P2 half\n    RHS R1 1.0\n",
    "probability '-0.5' is negative": BL + " BL B1 P2 -0.5\n    RHS R1 1.0\n",
    "probability 'nan' is negative or not finite": BL + " BL B1 P2 nan\n    RHS R1 1.0\n",
    r"BLOCKS keywords \['SUB'\]": "BLOCKS        SUB\n BL B1 P2 1.0\n    RHS R1 1.0\n",
    r"BLOCKS keywords \['LINTR'\]": "BLOCKS        LINTR\n",
    r"BLOCKS keywords \[\]": "BLOCKS\n",
    "before the first BL line": BL + "    RHS R1 1.0\n",
    "listed twice in its first realisation": BL + " BL B1 P2 1.0\n    RHS R1 1.0\n    RHS R1 2.0\n",
    "block B1 has no members": BL + " BL B1 P2 1.0\n",
    r"SCENARIOS keywords \['NORMAL'\]": "SCENARIOS     NORMAL\n",
    "parent 'S2' is not defined earlier": "SCENARIOS     DISCRETE\n SC S1 S2 0.5 P2\n    RHS R1 1.0\n SC S2 'ROOT' 0.5 P2\n    RHS R1 2.0\n",
    "scenario S1 defined twice": "SCENARIOS     DISCRETE\n SC S1 ROOT 0.5 P2\n    RHS R1 1.0\n SC S1 ROOT 0.5 P2\n    RHS R1 2.0\n",
    "scenario S1: probability '-1' is negative": "SCENARIOS     DISCRETE\n SC S1 ROOT -1 P2\n    RHS R1 1.0\n",
    "two-stage files only": "SCENARIOS     DISCRETE\n SC S1 ROOT 0.5 P2\n    RHS R1 1.0\n SC S2 S1 0.5 P3\n    RHS R1 2.0\n",
    "SCENARIOS cannot be combined with INDEP or BLOCKS": "INDEP DISCRETE\n    RHS R1 1.0 1.0\nSCENARIOS     DISCRETE\n SC S1 ROOT 1.0 P2\n    RHS R2 1.0\n",
    "cannot be combined with INDEP or BLOCKS": "SCENARIOS     DISCRETE\n SC S1 ROOT 1.0 P2\n    RHS R2 1.0\n" + BL + " BL B1 P2 1.0\n    RHS R1 1.0\n",
    "inherits from ROOT, which needs the core file": "SCENARIOS     DISCRETE\n SC S1 ROOT 0.5 P2\n    RHS R1 1.0\n SC S2 S1 0.5 P2\n    RHS R2 2.0\n",
}


@pytest.mark.parametrize("message", list(ERRORS))
def test_loader_errors(tmp_path, message):
    with pytest.raises(ValueError, match=message):
        smps.read_sto(_write(tmp_path, HEAD + ERRORS[message] + "ENDATA\n"))


def test_unknown_section_is_still_refused(tmp_path):
    with pytest.raises(AssertionError, match="unsupported STO section"):
        smps.read_sto(_write(tmp_path, HEAD + "CHANCE\nENDATA\n"))


def test_scenarios_inherit_along_the_parent_chain(tmp_path):
    """A position a scenario omits takes its parent's value, ROOT's being the core file's (quoted or
    not); without omissions from ROOT no core file is needed."""
    text = HEAD + ("SCENARIOS     DISCRETE\n SC A ROOT 0.5 P2\n    RHS R1 1.0\n    X1 R2 5.0\n SC B A 0.25 P2\n    X1 R2 6.0\n"
                   " SC C B 0.25 P2\n    RHS R1 3.0\nENDATA\n")
    sto = smps.read_sto(_write(tmp_path, text))
    b, = sto.blocks
    assert b.positions == [Pos("RHS", "R1"), Pos("X1", "R2")] and b.probs == [0.5, 0.25, 0.25]
    assert b.values == [[1.0, 5.0], [1.0, 6.0], [3.0, 6.0]]
    # lands3s' first scenario lists S2C5 only: S2C6 and S2C7 are lands' right-hand sides 3 and 2
    cor = smps.read_cor(os.path.join(DATA, "lands3s", "lands3s.cor"))
    assert cor.rhs[cor.row_mapping["S2C6"]] == 3.0 and cor.rhs[cor.row_mapping["S2C7"]] == 2.0
    assert smps.read_sto(os.path.join(DATA, "lands3s", "lands3s.sto"), cor).blocks[0].values[0] == [3.0, 3.0, 2.0]


# ---- the host helpers -------------------------------------------------------------------------------
def test_mean_joint_support_and_sample_values_on_lands3b():
    _, _, sto = smps.load_smps(os.path.join(DATA, "lands3b"))
    p, v = np.array(LANDS3_P), np.array(LANDS3_V, dtype=np.float64)
    np.testing.assert_allclose(smps.mean_values(sto), p @ v / p.sum(), rtol=1e-15)
    values, probs = smps.joint_support(sto)
    np.testing.assert_array_equal(values, v)
    np.testing.assert_array_equal(probs, p)
    back = [LANDS3_POS[2], LANDS3_POS[0], LANDS3_POS[1]]
    np.testing.assert_array_equal(smps.joint_support(sto, back)[0], v[:, [2, 0, 1]])
    with pytest.raises(ValueError, match="max_points"):
        smps.joint_support(sto, max_points=5)
    with pytest.raises(ValueError, match="whole blocks"):
        smps.joint_support(sto, LANDS3_POS[:2])
    with pytest.raises(ValueError, match="not a random element"):
        smps.joint_support(sto, LANDS3_POS + [Pos("RHS", "S2C1")])
    N = 4000
    draws = smps.sample_values(sto, N, np.random.default_rng(3))
    idx = np.array([np.nonzero((v == row).all(axis=1))[0] for row in draws])   # every row is one realisation
    assert idx.shape == (N, 1)
    freq = np.bincount(idx[:, 0], minlength=6) / N
    assert np.abs(freq - p).max() <= 4 * np.sqrt(0.25 / N)
    np.testing.assert_array_equal(smps.sample_values(sto, N, np.random.default_rng(3), back), draws[:, [2, 0, 1]])


def test_joint_support_is_the_product(tmp_path):
    text = HEAD + ("INDEP DISCRETE\n    RHS R1 1.0 0.5\n    RHS R1 2.0 0.25\n" + BL +
                   " BL B1 P2 0.5\n    RHS R2 10.0\n    RHS R3 20.0\n BL B1 P2 0.3\n    RHS R3 21.0\n BL B1 P2 0.2\n    RHS R2 12.0\n"
                   "INDEP DISCRETE\n    RHS R4 7.0 1.0\nENDATA\n")
    sto = smps.read_sto(_write(tmp_path, text))
    values, probs = smps.joint_support(sto)
    assert smps.sto_positions(sto) == [Pos("RHS", "R1"), Pos("RHS", "R4"), Pos("RHS", "R2"), Pos("RHS", "R3")]
    want = [[a, 7.0, b, c] for a in (1.0, 2.0) for b, c in ((10.0, 20.0), (10.0, 21.0), (12.0, 20.0))]
    np.testing.assert_array_equal(values, np.array(want))
    np.testing.assert_allclose(probs, [pa * pb for pa in (0.5, 0.25) for pb in (0.5, 0.3, 0.2)], rtol=1e-15)
    rows = smps.sample_values(sto, 500, np.random.default_rng(0))
    assert {tuple(r) for r in rows} <= {tuple(r) for r in want}
    # marginalising whole factors out
    v2, p2 = smps.joint_support(sto, [Pos("RHS", "R3"), Pos("RHS", "R2")])
    np.testing.assert_array_equal(v2, np.array([[20.0, 10.0], [21.0, 10.0], [20.0, 12.0]]))
    np.testing.assert_array_equal(p2, [0.5, 0.3, 0.2])


# ---- the library --------------------------------------------------------------------------------------
def test_library_exports_the_joint_entry_point():
    from sqlp_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "twosd_set_distributions_joint")
    assert ("twosd_set_distributions_joint" in [n for n, _, _ in _lib.SIGNATURES]) and _lib.DIST_BLOCK == 3
    with open(os.path.join(ROOT, "include", "twosd_hip.h")) as f:
        assert "#define TWOSD_DIST_BLOCK 3" in f.read()
