"""SMPS BLOCKS LINTR on the host: the loader's grammar and refusals, the layout,
mvnormal_lintr, joint_support, the restatement tests/lintr_ref.py, and the exact expectation of
data/smps/lands3t against the restated streams the GPU tests are written against.

lands3t at lands' x_EV (oracle LP, computed before the seed was fixed): exact expected recourse
252.076667; restated streams at seed 4242, N = 32768: i.i.d. z = -0.10 (standard error 0.2839),
antithetic z = 0.07 (0.0413), LHS 16 z = -0.30 (0.0512)."""
import os

import numpy as np
import pytest

from sqlp_amd import smps
from sqlp_amd.smps import spSmpsPosition as Pos
from tests import blocks_ref as B
from tests import lintr_ref as R
from tests import vr_ref as V

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "smps")
PLANS = ["iid", "antithetic", ("lhs", 8)]

GOOD = """STOCH         T
INDEP         UNIFORM
    RHS       R9        0.0       2.0
BLOCKS        LINTR
 BL B1        P2
    RHS       R3        10.0
    X1        R1        -2.0
    RHS       R2
 RV F         NORMAL    1.0       4.0
    RHS       R3        1.5
    X1        R1        -0.5
 RV G         DISCRETE
 SP 2.0       0.25
 SP -1.0      0.75
    X1        R1        2.0
    RHS       R2        0.0
 BL B2        P2
    RHS       R5        1.0
 RV U         UNIFORM   -1.0      3.0
    RHS       R5        0.25
BLOCKS        DISCRETE
 BL D1        P2        0.5
    RHS       R7        1.0
 BL D1        P2        0.5
    RHS       R7        2.0
ENDATA
"""


class _Cor:
    """What _template_value reads of a core file."""
    row_mapping = {"R2": 0}
    col_mapping = {}
    rhs = np.array([7.5])
    entries = {}


def _write(tmp_path, text, name="t.sto"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


# ---- the loader ---------------------------------------------------------------------------------------
def test_grammar(tmp_path):
    sto = smps.read_sto(_write(tmp_path, GOOD), _Cor())
    assert [b.name for b in sto.lintr] == ["B1", "B2"] and [b.name for b in sto.blocks] == ["D1"]
    b1, b2 = sto.lintr
    assert b1.period == "P2" and b1.positions == [Pos("RHS", "R3"), Pos("X1", "R1"), Pos("RHS", "R2")]
    assert b1.constants == [10.0, -2.0, 7.5]                       # the absent constant is the core file's value
    assert b1.latent_names == ["F", "G"]
    assert b1.latents == [("NORMAL", 1.0, 4.0), ("DISCRETE", [2.0, -1.0], [0.25, 0.75])]
    assert b1.rows == [[(0, 1.5)], [(0, -0.5), (1, 2.0)], [(1, 0.0)]]       # an explicit zero is kept
    assert b2.positions == [Pos("RHS", "R5")] and b2.constants == [1.0] and b2.latents == [("UNIFORM", -1.0, 3.0)]
    assert b2.rows == [[(0, 0.25)]]
    # the layout: INDEP, the discrete blocks' members, then the LINTR members
    assert smps.sto_positions(sto) == [Pos("RHS", "R9"), Pos("RHS", "R7")] + b1.positions + b2.positions
    # means: c + H E xi
    mu = smps.mean_values(sto)
    np.testing.assert_allclose(mu, [1.0, 1.5, 10.0 + 1.5 * 1.0, -2.0 - 0.5 * 1.0 + 2.0 * -0.25, 7.5, 1.0 + 0.25 * 1.0], rtol=1e-15)
    # the absent constant needs the core file
    with pytest.raises(ValueError, match="core file"):
        smps.read_sto(_write(tmp_path, GOOD))
    # host sampling: members are affine in the block's latents
    v = smps.sample_values(sto, 4000, np.random.default_rng(5))
    assert v.shape == (4000, 6)
    xi_g = (v[:, 4] - 7.5)                                         # 0 * G: the member is its constant
    assert (xi_g == 0.0).all()
    f = (v[:, 2] - 10.0) / 1.5
    g = (v[:, 3] + 2.0 + 0.5 * f) / 2.0
    assert set(np.round(g, 9)) == {2.0, -1.0}
    assert abs(f.mean() - 1.0) < 0.2 and abs(f.std() - 2.0) < 0.2
    assert ((v[:, 5] - 1.0) / 0.25 >= -1.0).all() and ((v[:, 5] - 1.0) / 0.25 <= 3.0).all()


def _edit(old, new):
    assert old in GOOD
    return GOOD.replace(old, new, 1)


REFUSALS = {
    "is no member": _edit("    RHS       R3        1.5\n", "    RHS       R8        1.5\n"),
    "member .* listed twice": _edit("    X1        R1        -2.0\n", "    X1        R1        -2.0\n    RHS       R3        1.0\n"),
    "RV F has no coefficient lines": _edit("    RHS       R3        1.5\n    X1        R1        -0.5\n", ""),
    "listed twice under RV F": _edit("    X1        R1        -0.5\n", "    X1        R1        -0.5\n    X1        R1        0.5\n"),
    "RV G has no SP lines": _edit(" SP 2.0       0.25\n SP -1.0      0.75\n", ""),
    "RV F defined twice": _edit(" RV G         DISCRETE\n", " RV F         DISCRETE\n"),
    "before any member line": _edit("    RHS       R5        1.0\n", ""),
    "has no RV": _edit(" RV U         UNIFORM   -1.0      3.0\n    RHS       R5        0.25\n", ""),
    "needs two parameters": _edit(" RV U         UNIFORM   -1.0      3.0\n", " RV U         UNIFORM   -1.0\n"),
    "SP line outside a DISCRETE RV": _edit("    RHS       R3        1.5\n", " SP 1.0       0.5\n    RHS       R3        1.5\n"),
    "probability .* negative": _edit(" SP 2.0       0.25\n", " SP 2.0       -0.25\n"),
    "is not a number": _edit("    RHS       R3        1.5\n", "    RHS       R3        abc\n"),
    "after the block's first BL line": _edit(" BL B2        P2\n", " BL B1        P2\n"),
    "period 'P3' after 'P2'": _edit(" BL B2        P2\n", " BL B1        P3\n"),
    "is in LINTR block B2 and in INDEP": _edit("    RHS       R5        1.0\n", "    RHS       R9        1.0\n").replace(
        "    RHS       R5        0.25\n", "    RHS       R9        0.25\n"),
    "is in blocks B1 and B2": _edit("    RHS       R5        1.0\n", "    RHS       R3        1.0\n").replace(
        "    RHS       R5        0.25\n", "    RHS       R3        0.25\n"),
    "is in blocks D1 and B2": _edit("    RHS       R5        1.0\n", "    RHS       R7        1.0\n").replace(
        "    RHS       R5        0.25\n", "    RHS       R7        0.25\n"),
    "line before the first BL line": _edit(" BL B1        P2\n    RHS       R3        10.0\n", "    RHS       R3        10.0\n"),
    "unsupported BLOCKS keywords": _edit("BLOCKS        LINTR\n", "BLOCKS        SUB\n"),
    "the section holds no BL line": _edit("BLOCKS        DISCRETE\n", "BLOCKS        LINTR\nBLOCKS        DISCRETE\n"),
    r"BLOCKS keywords \['LINTR'\]: the section holds no BL line": "STOCH         T\nBLOCKS        LINTR\n",
}


@pytest.mark.parametrize("message", list(REFUSALS))
def test_loader_refusals(tmp_path, message):
    with pytest.raises(ValueError, match=message):
        smps.read_sto(_write(tmp_path, REFUSALS[message]), _Cor())


def test_a_reopened_block_takes_more_latents(tmp_path):
    text = _edit(" BL B2        P2\n    RHS       R5        1.0\n RV U ", " BL B1        P2\n RV U ").replace(
        "    RHS       R5        0.25\n", "    RHS       R2        0.25\n")
    sto = smps.read_sto(_write(tmp_path, text), _Cor())
    b, = sto.lintr
    assert b.latent_names == ["F", "G", "U"] and b.rows[2] == [(1, 0.0), (2, 0.25)]


def test_lands3t_layout_and_joint_support():
    cor, tim, sto = smps.load_smps(os.path.join(DATA, "lands3t"))
    assert sto.indep == {} and sto.blocks == [] and len(sto.lintr) == 1
    b = sto.lintr[0]
    assert b.name == "DEMAND" and b.period == "PERIOD2"
    assert b.positions == [Pos("RHS", "S2C5"), Pos("RHS", "S2C6"), Pos("RHS", "S2C7")]
    assert b.constants == [5.0, 3.0, 2.0]
    assert b.latents == [("DISCRETE", [-1.0, 0.0, 1.0], [0.3, 0.4, 0.3]), ("DISCRETE", [0.0, 1.0], [0.6, 0.4])]
    assert b.rows == [[(0, 1.0)], [(0, 0.5), (1, -1.0)], [(0, 0.5), (1, 1.0)]]        # one shared column, one partial
    sp2 = smps.get_smps_stage_template(cor, tim, 2)
    pos, rows, cols = smps.scenario_positions(sp2, sto)
    assert pos == b.positions and rows.tolist() == [4, 5, 6] and cols.tolist() == [-1, -1, -1]
    for ext in ("cor", "tim"):
        a = open(os.path.join(DATA, "lands3b", f"lands3b.{ext}")).read()
        assert open(os.path.join(DATA, "lands3t", f"lands3t.{ext}")).read() == a.replace("LandS3b", "LandS3t", 1)
    values, probs = smps.joint_support(sto)
    assert values.shape == (6, 3) and probs.shape == (6,)
    np.testing.assert_array_equal(probs, np.array([0.3, 0.3, 0.4, 0.4, 0.3, 0.3]) * np.array([0.6, 0.4] * 3))   # probabilities multiply
    np.testing.assert_array_equal(values, [[4, 2.5, 1.5], [4, 1.5, 2.5], [5, 3, 2], [5, 2, 3], [6, 3.5, 2.5], [6, 2.5, 3.5]])
    # every joint point lies inside the per-row range of lands3b's realisations
    vb = np.asarray(smps.load_smps(os.path.join(DATA, "lands3b"))[2].blocks[0].values)
    assert (values >= vb.min(axis=0)).all() and (values <= vb.max(axis=0)).all()
    np.testing.assert_allclose(smps.mean_values(sto), probs @ values, rtol=1e-15)
    # a continuous latent has no joint support
    sto.lintr[0].latents[1] = ("UNIFORM", 0.0, 1.0)
    with pytest.raises(ValueError, match="not DISCRETE"):
        smps.joint_support(sto)


def test_mvnormal_lintr():
    sd = np.array([2.0, 0.5, 3.0])
    corr = np.array([[1.0, 0.8, -0.3], [0.8, 1.0, 0.1], [-0.3, 0.1, 1.0]])
    cov = corr * np.outer(sd, sd)
    pos = [("RHS", "A"), ("RHS", "B"), ("X", "C")]
    b = smps.mvnormal_lintr("MVN", "P2", pos, [1.0, -2.0, 0.5], cov)
    assert b.positions == [Pos(*p) for p in pos] and b.constants == [1.0, -2.0, 0.5]
    assert b.latents == [("NORMAL", 0.0, 1.0)] * 3 and [[l for l, _ in r] for r in b.rows] == [[0], [0, 1], [0, 1, 2]]
    H = np.zeros((3, 3))
    for j, row in enumerate(b.rows):
        for l, h in row:
            H[j, l] = h
    assert np.abs(H @ H.T - cov).max() <= 1e-14 * np.abs(cov).max()
    with pytest.raises(ValueError, match="positive definite"):
        smps.mvnormal_lintr("MVN", "P2", pos, [0, 0, 0], [[1, 2, 0], [2, 1, 0], [0, 0, 1]])
    with pytest.raises(ValueError, match="symmetric"):
        smps.mvnormal_lintr("MVN", "P2", pos, [0, 0, 0], [[1, 0.5, 0], [0.2, 1, 0], [0, 0, 1]])


# ---- the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", PLANS)
def test_identity_block_reproduces_the_latents(plan):
    """H = I, c = 0: the members are the latents, i.e. columns k .. k+Q-1 of the independent stream
    of k + Q elements; the other columns are those of the layout without the block."""
    lat = [("DISCRETE", [1.0, 4.0, 2.0], [0.3, 0.3, 0.3]), ("UNIFORM", -1.0, 3.0), ("NORMAL", 10.0, 4.0)]
    dists = [("UNIFORM", 0.0, 2.0), ("LINTR",), ("NORMAL", -3.0, 0.25), ("LINTR",), ("LINTR",)]
    lintr = [([4, 1, 3], [0.0, 0.0, 0.0], lat, [[(0, 1.0)], [(1, 1.0)], [(2, 1.0)]])]
    N, seed, first = 64, 0x5EED1234ABCDEF, 2 ** 32 - 32
    got = R.draw(plan, dists, [], lintr, N, seed, first)
    layout = [("UNIFORM", 0.0, 2.0), ("UNIFORM", 5.0, 6.0), ("NORMAL", -3.0, 0.25), ("UNIFORM", 5.0, 6.0), ("UNIFORM", 5.0, 6.0)] + lat
    if plan == "iid":
        ext = V.iid(layout, N, seed, first)
    elif plan == "antithetic":
        ext = V.antithetic(layout, N, seed, first)
    else:
        ext = V.lhs(layout, plan[1], N, seed, first)
    np.testing.assert_array_equal(got[:, [4, 1, 3]], 0.0 + 1.0 * ext[:, 5:8])
    np.testing.assert_array_equal(got[:, [0, 2]], ext[:, [0, 2]])
    assert len(np.unique(got[:, 4])) == 3


def test_a_file_without_lintr_keeps_its_layout():
    for name in ("lands", "lands3b", "lands3s", "storm"):
        sto = smps.load_smps(os.path.join(DATA, name))[2]
        assert sto.lintr == []
        assert smps.sto_positions(sto) == list(sto.indep.keys()) + [p for b in sto.blocks for p in b.positions]
        dists, blocks, lintr = R.table_of(sto, smps.sto_positions(sto))
        assert lintr == [] and (dists, [b[0] for b in blocks]) == (B.table_of(sto, smps.sto_positions(sto))[0],
                                                                     [b[0] for b in B.table_of(sto, smps.sto_positions(sto))[1]])


# ---- lands3t: the exact expectation covers the restated streams ---------------------------------------
@pytest.mark.parametrize("plan", R.LANDS3T_PLANS)
def test_lands3t_restated_streams_cover_the_exact_expectation(plan):
    L = R.lands3t()
    assert abs(L["exact"] - 252.076667) <= 1e-6
    s = L["streams"][plan]
    z = (s["mean"] - L["exact"]) / s["se"]
    print(f"{plan}: mean {s['mean']:.6f}, exact {L['exact']:.6f}, standard error {s['se']:.4f}, z = {z:.2f}")
    assert abs(z) <= 4.0


def test_library_exports_the_lintr_entry_point_in_its_header():
    """The header declares what the binding lists (the symbol itself is checked on the GPU machine,
    where the library is loaded)."""
    from sqlp_amd import _lib
    root = os.path.dirname(os.path.dirname(DATA))
    text = open(os.path.join(root, "include", "twosd_hip.h")).read()
    assert "int twosd_set_distributions_lintr(" in text and "#define TWOSD_DIST_LINTR 4" in text
    sig = dict((n, a) for n, _, a in _lib.SIGNATURES)["twosd_set_distributions_lintr"]
    assert len(sig) == 15 and _lib.DIST_LINTR == 4
    assert [f for f, _ in _lib.Lintr._fields_] == ["nblocks", "member_off", "members", "constants", "latent_off", "latent_kind",
                                                    "latent_nsupport", "latent_values", "latent_probs", "latent_param0",
                                                    "latent_param1", "row_ptr", "col", "val"]
