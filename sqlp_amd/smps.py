"""SMPS reader + stage split (host plumbing that feeds the hot path).

Mirrors the reference's reader (names and semantics):
  read_cor                 src/smps/smps_cor.jl:160-194 (tokenizer :26-58, bounds :124-155)
  read_tim                 src/smps/smps_tim.jl:30-64
  read_sto                 src/smps/smps_sto.jl:41-110 (INDEP); BLOCKS DISCRETE, BLOCKS LINTR and
                           two-stage SCENARIOS DISCRETE have no reference counterpart
                           (data/smps/README.md)
  get_smps_stage_template  src/smps/smps_prob.jl:14-102
  rand(sto)                src/smps/smps_sto.jl:117-149 (DISCRETE / NORMAL(mean, variance) /
                           UNIFORM), here vectorised with numpy's PCG64 -- Julia's RNG
                           streams cannot be reproduced, so samples are not bitwise Julia's.
The product keeps everything sparse (CSC arrays ready for twosd_set_template).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np


class spSmpsPosition(NamedTuple):
    """(col_name, row_name) of a random element; col 'RHS'/'rhs' marks an RHS entry."""
    col_name: str
    row_name: str


@dataclass
class spCorType:
    problem_name: str
    directions: list
    row_names: list
    col_names: list
    entries: dict            # (row, col) -> value, last assignment wins
    rhs: np.ndarray
    lower_bound: np.ndarray
    upper_bound: np.ndarray
    col_mapping: dict
    row_mapping: dict


@dataclass
class spSmpsImplicitPeriod:
    period_name: str
    position: spSmpsPosition


@dataclass
class spTimType:
    problem_name: str
    periods: list


@dataclass
class spStoBlock:
    """A joint discrete distribution: realisation r has probability probs[r] and gives member
    positions[j] the value values[r][j].  Realisations keep the file's order; nothing is sorted,
    merged or normalised."""
    name: str
    period: str
    positions: list          # spSmpsPosition, in first-appearance order
    probs: list              # R
    values: list             # R rows of len(positions)


@dataclass
class spStoLintr:
    """A LINTR block: member positions[j] = constants[j] + sum_l H[j][l] xi_l over independent
    latent variables.  latents[l] is ("DISCRETE", values, probs) / ("NORMAL", mean, variance) /
    ("UNIFORM", left, right), an entry of spStoType.indep; rows[j] lists the entries (l, h) of row j
    of H with l ascending, kept as the file gives them (explicit zeros included)."""
    name: str
    period: str
    positions: list          # spSmpsPosition, in the order of the first BL line's member lines
    constants: list          # n
    latent_names: list       # q
    latents: list            # q
    rows: list               # n lists of (latent index, coefficient)


@dataclass
class spStoType:
    problem_name: str
    indep: dict = field(default_factory=dict)   # position -> (kind, a, b); insertion ordered
    blocks: list = field(default_factory=list)  # spStoBlock, file order
    lintr: list = field(default_factory=list)   # spStoLintr, file order


def _lines(path):
    with open(path, "r", encoding="latin-1") as f:
        return f.read().splitlines()


def read_cor(path) -> spCorType:
    sections = ("NAME", "ROWS", "COLUMNS", "RHS", "BOUNDS", "ENDATA")
    tok = {s: [] for s in sections}
    section = ""
    for line in _lines(path):
        if not line or line[0] == '*':
            continue
        t = line.split()
        if line[0] != ' ':
            section = t[0]
            if section not in sections:
                raise AssertionError(f"unsupported COR section {section!r}")
            if section == "NAME":
                tok["NAME"].append(t[1])          # BoundsError in the reference if missing
        else:
            tok[section].append(t)
    directions = [t[0][0] for t in tok["ROWS"]]
    row_names = [t[1] for t in tok["ROWS"]]
    col_names = list(dict.fromkeys(t[0] for t in tok["COLUMNS"]))
    rowm = {r: i for i, r in enumerate(row_names)}
    colm = {c: j for j, c in enumerate(col_names)}
    entries = {}
    for t in tok["COLUMNS"]:
        j = colm[t[0]]
        for a in range(1, len(t) - 1, 2):
            v = float(t[a + 1])
            key = (rowm[t[a]], j)
            if v != 0.0:
                entries[key] = v
            else:
                entries.pop(key, None)
    rhs = np.zeros(len(row_names))
    for t in tok["RHS"]:
        for a in range(1, len(t) - 1, 2):
            rhs[rowm[t[a]]] = float(t[a + 1])
    lb = np.zeros(len(col_names))
    ub = np.full(len(col_names), np.inf)
    for t in tok["BOUNDS"]:
        bt = t[0]
        if bt not in ("LO", "UP", "FX", "FR", "MI", "PL"):
            raise AssertionError(f"Unsupported bound type {bt} for variable {t[2]}")
        j = colm[t[2]]
        if bt == "LO":
            lb[j] = float(t[3])
        elif bt == "UP":
            ub[j] = float(t[3])
        elif bt == "FX":
            lb[j] = ub[j] = float(t[3])
        elif bt == "FR":
            lb[j], ub[j] = -np.inf, np.inf
        elif bt == "MI":
            lb[j] = -np.inf
        else:
            ub[j] = np.inf
    if not directions or directions[0] != 'N':
        raise AssertionError(f"First row or cor file is not objective. {''.join(directions)}")
    return spCorType(tok["NAME"][0], directions, row_names, col_names, entries, rhs, lb, ub, colm, rowm)


def read_tim(path) -> spTimType:
    name, periods, section = "", [], ""
    for line in _lines(path):
        t = line.split()
        if line[0] == ' ':
            if section != "PERIODS":
                raise AssertionError("TIM data line outside PERIODS")
            periods.append(spSmpsImplicitPeriod(t[2], spSmpsPosition(t[0], t[1])))
        else:
            section = t[0]
            if section not in ("TIME", "PERIODS", "ENDATA"):
                raise AssertionError(f"unsupported TIM section {section!r}")
            if section == "TIME":
                name = t[1]
    return spTimType(name, periods)


def _probability(tok, what):
    try:
        p = float(tok)
    except ValueError:
        raise ValueError(f"{what}: probability {tok!r} is not a number") from None
    if not p >= 0.0 or p == float("inf"):
        raise ValueError(f"{what}: probability {tok!r} is negative or not finite")
    return p


def _template_value(cor, pos, who="SCENARIOS"):
    """The core file's value at a random position (RHS entry or matrix coefficient)."""
    if cor is None:
        raise ValueError(f"{who}: {tuple(pos)} takes the core file's value, which needs the core file (read_sto(path, cor))"
                         if who != "SCENARIOS" else
                         f"SCENARIOS: {tuple(pos)} inherits from ROOT, which needs the core file (read_sto(path, cor))")
    i = cor.row_mapping[pos.row_name]
    if pos.col_name in ("RHS", "rhs"):
        return float(cor.rhs[i])
    return float(cor.entries.get((i, cor.col_mapping[pos.col_name]), 0.0))


def _number(tok, what):
    try:
        return float(tok)
    except ValueError:
        raise ValueError(f"{what}: {tok!r} is not a number") from None


def _read_lintr_line(st, t, line, cor):
    """One data line of a BLOCKS LINTR section (grammar: data/smps/README.md).  st: the section's
    state, {"blocks": name -> spStoLintr, "cur": the open block, "rv": its open latent index or None,
    "members_open": member lines still allowed}."""
    if t[0] == "BL" and len(t) == 3:
        name, period = t[1], t[2]
        new = name not in st["blocks"]
        if new:
            st["blocks"][name] = spStoLintr(name, period, [], [], [], [], [])
            st["order"].append(st["blocks"][name])
        b = st["blocks"][name]
        if b.period != period:
            raise ValueError(f"LINTR block {name}: period {period!r} after {b.period!r}")
        st.update(cur=b, rv=None, members_open=new)    # the first BL line of a block fixes its members
        return
    b = st["cur"]
    if b is None:
        raise ValueError(f"BLOCKS LINTR: line before the first BL line: {line.strip()!r}")
    if t[0] == "RV" and len(t) >= 3 and t[2] in ("NORMAL", "UNIFORM", "DISCRETE"):
        name, kind = t[1], t[2]
        if not b.positions:
            raise ValueError(f"LINTR block {b.name}: RV {name} before any member line")
        if name in b.latent_names:
            raise ValueError(f"LINTR block {b.name}: RV {name} defined twice")
        if kind == "DISCRETE":
            if len(t) != 3:
                raise ValueError(f"LINTR block {b.name}: RV {name} DISCRETE takes no parameters: {line.strip()!r}")
            b.latents.append(("DISCRETE", [], []))
        else:
            if len(t) != 5:
                raise ValueError(f"LINTR block {b.name}: RV {name} {kind} needs two parameters: {line.strip()!r}")
            b.latents.append((kind, _number(t[3], f"RV {name}"), _number(t[4], f"RV {name}")))
        b.latent_names.append(name)
        st.update(rv=len(b.latents) - 1, members_open=False)
        return
    if t[0] == "SP" and len(t) == 3:
        if st["rv"] is None or b.latents[st["rv"]][0] != "DISCRETE":
            raise ValueError(f"LINTR block {b.name}: SP line outside a DISCRETE RV: {line.strip()!r}")
        if any(st["rv"] == l for row in b.rows for l, _ in row):
            raise ValueError(f"LINTR block {b.name}: SP line after the coefficient lines of RV {b.latent_names[st['rv']]}")
        b.latents[st["rv"]][1].append(_number(t[1], f"RV {b.latent_names[st['rv']]}"))
        b.latents[st["rv"]][2].append(_probability(t[2], f"RV {b.latent_names[st['rv']]}"))
        return
    if len(t) not in (2, 3):
        raise ValueError(f"BLOCKS LINTR: cannot read {line.strip()!r}")
    pos = spSmpsPosition(t[0], t[1])
    if st["rv"] is None:                               # a member line
        if not st["members_open"]:
            raise ValueError(f"LINTR block {b.name}: member line {tuple(pos)} after the block's first BL line was closed")
        if pos in b.positions:
            raise ValueError(f"LINTR block {b.name}: member {tuple(pos)} listed twice")
        b.positions.append(pos)
        b.constants.append(_number(t[2], f"member {tuple(pos)}") if len(t) == 3 else _template_value(cor, pos, "BLOCKS LINTR"))
        b.rows.append([])
        return
    if pos not in b.positions:                         # a coefficient line of the open RV
        raise ValueError(f"LINTR block {b.name}: coefficient of {tuple(pos)}, which is no member")
    if len(t) != 3:
        raise ValueError(f"LINTR block {b.name}: coefficient line without a value: {line.strip()!r}")
    row = b.rows[b.positions.index(pos)]
    if row and row[-1][0] == st["rv"]:
        raise ValueError(f"LINTR block {b.name}: {tuple(pos)} listed twice under RV {b.latent_names[st['rv']]}")
    row.append((st["rv"], _number(t[2], f"coefficient of {tuple(pos)}")))


def _check_lintr(b):
    if not b.positions:
        raise ValueError(f"LINTR block {b.name} has no members")
    if not b.latents:
        raise ValueError(f"LINTR block {b.name} has no RV")
    used = {l for row in b.rows for l, _ in row}
    for l, (name, d) in enumerate(zip(b.latent_names, b.latents)):
        if l not in used:
            raise ValueError(f"LINTR block {b.name}: RV {name} has no coefficient lines")
        if d[0] == "DISCRETE" and not d[1]:
            raise ValueError(f"LINTR block {b.name}: DISCRETE RV {name} has no SP lines")


def read_sto(path, cor: spCorType = None) -> spStoType:
    """INDEP (DISCRETE / NORMAL / UNIFORM), BLOCKS DISCRETE, BLOCKS LINTR and two-stage SCENARIOS
    DISCRETE.  Several INDEP and BLOCKS sections may follow each other in any order; SCENARIOS stands
    alone.  `cor` supplies the values a SCENARIOS scenario inherits from ROOT and the constant of a
    LINTR member line that gives none."""
    sto = spStoType("")
    lintr = {"blocks": {}, "order": sto.lintr, "cur": None, "rv": None, "members_open": False}
    section, kw = "", []
    blocks = {}                 # name -> spStoBlock (BLOCKS)
    cur = None                  # (block, realisation row) the value lines go to
    scen, scen_pos, scen_cur = {}, [], None   # SCENARIOS: name -> [parent, prob, period, {pos: value}]
    seen = set()
    for line in _lines(path):
        if not line or line[0] == '*':
            continue
        t = line.split()
        if line[0] == ' ':
            if section == "BLOCKS" and kw == ["LINTR"]:
                _read_lintr_line(lintr, t, line, cor)
                continue
            if section == "BLOCKS":
                if t[0] == "BL" and len(t) == 4:
                    name, period, p = t[1], t[2], _probability(t[3], f"block {t[1]}")
                    if name not in blocks:
                        blocks[name] = spStoBlock(name, period, [], [], [])
                        sto.blocks.append(blocks[name])
                    b = blocks[name]
                    if b.period != period:
                        raise ValueError(f"block {name}: period {period!r} after {b.period!r}")
                    b.probs.append(p)
                    b.values.append(list(b.values[0]) if b.values else [])   # omitted members: the first realisation's
                    cur = b
                    continue
                if cur is None:
                    raise ValueError(f"BLOCKS: value line before the first BL line: {line.strip()!r}")
                pos, v = spSmpsPosition(t[0], t[1]), float(t[2])
                if len(cur.values) == 1:          # the first realisation fixes the members and their order
                    if pos in cur.positions:
                        raise ValueError(f"block {cur.name}: {tuple(pos)} listed twice in its first realisation")
                    cur.positions.append(pos)
                    cur.values[0].append(v)
                elif pos not in cur.positions:
                    raise ValueError(f"block {cur.name}: {tuple(pos)} is absent from its first realisation")
                else:
                    cur.values[-1][cur.positions.index(pos)] = v
                continue
            if section == "SCENARIOS":
                if t[0] == "SC" and len(t) == 5:
                    name, parent, p = t[1], t[2].strip("'"), _probability(t[3], f"scenario {t[1]}")
                    if name in scen:
                        raise ValueError(f"scenario {name} defined twice")
                    if parent != "ROOT" and parent not in scen:
                        raise ValueError(f"scenario {name}: parent {parent!r} is not defined earlier in the file")
                    scen[name] = scen_cur = [parent, p, t[4], {}]
                    continue
                if scen_cur is None:
                    raise ValueError(f"SCENARIOS: value line before the first SC line: {line.strip()!r}")
                pos = spSmpsPosition(t[0], t[1])
                if pos not in scen_pos:
                    scen_pos.append(pos)
                scen_cur[3][pos] = float(t[2])
                continue
            if section != "INDEP":
                continue
            if len(kw) > 1:
                raise ValueError(f"Trailing/unsupported section_keywords {kw}")
            pos = spSmpsPosition(t[0], t[1])
            if kw[0] == "UNIFORM":
                sto.indep[pos] = ("UNIFORM", float(t[2]), float(t[3]))
            elif kw[0] == "NORMAL":
                sto.indep[pos] = ("NORMAL", float(t[2]), float(t[3]))
            elif kw[0] == "DISCRETE":
                if pos not in sto.indep:
                    sto.indep[pos] = ("DISCRETE", [], [])
                sto.indep[pos][1].append(float(t[2]))
                sto.indep[pos][2].append(float(t[3]))
            else:
                raise ValueError(f"Unknown or unsupported section_keywords {kw}")
        else:
            if section == "BLOCKS" and kw == ["LINTR"] and lintr["cur"] is None:
                # a LINTR section must state a block: a bare keyword line says nothing that can be read
                raise ValueError(f"BLOCKS keywords {kw}: the section holds no BL line")
            section = t[0]
            if section not in ("STOCH", "INDEP", "BLOCKS", "SCENARIOS", "ENDATA"):
                raise AssertionError(f"unsupported STO section {section!r}")
            kw = t[1:]
            cur = None
            lintr.update(cur=None, rv=None, members_open=False)
            seen.add(section)
            if section == "STOCH":
                sto.problem_name = kw[0]
            elif section == "BLOCKS" and kw == ["LINTR"]:
                pass
            elif section in ("BLOCKS", "SCENARIOS") and kw != ["DISCRETE"]:
                raise ValueError(f"unsupported {section} keywords {kw}: only DISCRETE{' and LINTR are' if section == 'BLOCKS' else ' is'} read")
            if "SCENARIOS" in seen and ("INDEP" in seen or "BLOCKS" in seen):
                raise ValueError("SCENARIOS cannot be combined with INDEP or BLOCKS in one file")
    if section == "BLOCKS" and kw == ["LINTR"] and lintr["cur"] is None:      # a file that ends without ENDATA
        raise ValueError(f"BLOCKS keywords {kw}: the section holds no BL line")
    if scen:
        # one block over the union of the positions, one realisation per scenario; a position a
        # scenario omits takes its parent's value, ROOT's being the core file's
        rows = {}
        for name, (parent, _, _, given) in scen.items():
            base = rows[parent] if parent != "ROOT" else None
            rows[name] = [given[pos] if pos in given else base[j] if base is not None else _template_value(cor, pos)
                          for j, pos in enumerate(scen_pos)]
        periods = {v[2] for v in scen.values()}
        if len(periods) > 1:
            raise ValueError(f"SCENARIOS: two-stage files only, found periods {sorted(periods)}")
        sto.blocks.append(spStoBlock("SCENARIOS", periods.pop(), scen_pos, [v[1] for v in scen.values()],
                                     [rows[name] for name in scen]))
    owner = {}
    for b in sto.blocks:
        if not b.positions:
            raise ValueError(f"block {b.name} has no members")
        for pos in b.positions:
            if pos in sto.indep:
                raise ValueError(f"{tuple(pos)} is in block {b.name} and in INDEP")
            if pos in owner:
                raise ValueError(f"{tuple(pos)} is in blocks {owner[pos]} and {b.name}")
            owner[pos] = b.name
    for b in sto.lintr:
        _check_lintr(b)
        for pos in b.positions:
            if pos in sto.indep:
                raise ValueError(f"{tuple(pos)} is in LINTR block {b.name} and in INDEP")
            if pos in owner:
                raise ValueError(f"{tuple(pos)} is in blocks {owner[pos]} and {b.name}")
            owner[pos] = b.name
    return sto


@dataclass
class spStageProblem:
    """Sparse stage problem: rows (W y + T x) {G,L,E} r, objective q'y (MIN)."""
    last_stage_vars: list
    current_stage_vars: list
    stage_constraints: list
    sense: list
    q: np.ndarray
    r: np.ndarray
    T: tuple           # CSC (colptr, rowval, nzval), m x n1, 0-based int64
    W: tuple           # CSC m x n2
    ylb: np.ndarray
    yub: np.ndarray

    @property
    def shape(self):
        return len(self.stage_constraints), len(self.last_stage_vars), len(self.current_stage_vars)

    def dense_T(self):
        return _csc_dense(self.T, len(self.stage_constraints), len(self.last_stage_vars))

    def dense_W(self):
        return _csc_dense(self.W, len(self.stage_constraints), len(self.current_stage_vars))


def _csc(entries, rows, cols):
    ri = {r: i for i, r in enumerate(rows)}
    colptr = [0]
    rv, nz = [], []
    for c in cols:
        col = sorted((ri[r], v) for (r, cc), v in entries.items() if cc == c and r in ri)
        rv += [i for i, _ in col]
        nz += [v for _, v in col]
        colptr.append(len(rv))
    return (np.array(colptr, dtype=np.int64), np.array(rv, dtype=np.int64), np.array(nz, dtype=np.float64))


def _csc_dense(csc, m, n):
    cp, rv, nz = csc
    A = np.zeros((m, n))
    for j in range(n):
        A[rv[cp[j]:cp[j + 1]], j] = nz[cp[j]:cp[j + 1]]
    return A


def get_smps_stage_template(cor: spCorType, tim: spTimType, stage: int) -> spStageProblem:
    P = tim.periods
    assert 1 <= stage <= len(P)
    start_col = 0 if stage == 1 else cor.col_mapping[P[stage - 2].position.col_name]
    end_col = cor.col_mapping[P[stage].position.col_name] - 1 if stage < len(P) else len(cor.col_names) - 1
    cur_start = cor.col_mapping[P[stage - 1].position.col_name]
    start_row = 1 if stage == 1 else cor.row_mapping[P[stage - 1].position.row_name]
    end_row = cor.row_mapping[P[stage].position.row_name] - 1 if stage < len(P) else len(cor.row_names) - 1
    last = list(range(start_col, cur_start))
    cur = list(range(cur_start, end_col + 1))
    rows = list(range(start_row, end_row + 1))
    # column-sliced entries
    by_col = {}
    for (i, j), v in cor.entries.items():
        by_col.setdefault(j, []).append((i, v))
    rowpos = {r: p for p, r in enumerate(rows)}

    def csc_of(cols):
        colptr, rv, nz = [0], [], []
        for j in cols:
            col = sorted((rowpos[i], v) for i, v in by_col.get(j, []) if i in rowpos)
            rv += [i for i, _ in col]
            nz += [v for _, v in col]
            colptr.append(len(rv))
        return (np.array(colptr, dtype=np.int64), np.array(rv, dtype=np.int64), np.array(nz, dtype=np.float64))

    q = np.array([cor.entries.get((0, j), 0.0) for j in cur])
    return spStageProblem(
        last_stage_vars=[cor.col_names[j] for j in last],
        current_stage_vars=[cor.col_names[j] for j in cur],
        stage_constraints=[cor.row_names[i] for i in rows],
        sense=[cor.directions[i] for i in rows],
        q=q, r=cor.rhs[rows].copy(), T=csc_of(last), W=csc_of(cur),
        ylb=cor.lower_bound[cur].copy(), yub=cor.upper_bound[cur].copy())


def load_smps(directory, name=None):
    """(cor, tim, sto) of an SMPS triple <dir>/<name>.{cor,tim,sto}."""
    name = name or os.path.basename(os.path.normpath(directory))
    base = os.path.join(directory, name)
    cor = read_cor(base + ".cor")
    return cor, read_tim(base + ".tim"), read_sto(base + ".sto", cor)


# ---------------------------------------------------------------------- scenarios
def sto_positions(sto: spStoType) -> list:
    """The random-element layout of a sto: the INDEP positions, then every block's members in
    file order, then every LINTR block's members (on a file without blocks: the INDEP positions as
    before; without LINTR blocks: the layout as before them)."""
    return (list(sto.indep.keys()) + [p for b in sto.blocks for p in b.positions] +
            [p for b in getattr(sto, "lintr", []) for p in b.positions])


def _block_members(sto: spStoType) -> dict:
    """position -> (block index, member column)"""
    return {p: (bi, j) for bi, b in enumerate(sto.blocks) for j, p in enumerate(b.positions)}


def _lintr_members(sto: spStoType) -> dict:
    """position -> (LINTR block index, member row)"""
    return {p: (bi, j) for bi, b in enumerate(getattr(sto, "lintr", [])) for j, p in enumerate(b.positions)}


def lintr_apply(b: spStoLintr, xi: np.ndarray) -> np.ndarray:
    """Member values (N, n) of a LINTR block at latent values xi (N, q): v = c_j, then
    v = v + (h * xi_l) for the entries of row j in order -- elementwise numpy, so every product and
    every sum is one fp64 rounding, as on the device."""
    xi = np.asarray(xi, dtype=np.float64)
    out = np.empty((xi.shape[0], len(b.positions)))
    for j, row in enumerate(b.rows):
        v = np.full(xi.shape[0], float(b.constants[j]))
        for l, h in row:
            v = v + float(h) * xi[:, l]
        out[:, j] = v
    return out


def _latent_moments(d):
    """(mean, variance) of a latent."""
    if d[0] == "DISCRETE":
        v, p = np.asarray(d[1], dtype=np.float64), np.asarray(d[2], dtype=np.float64)
        mu = float(np.dot(p, v) / np.sum(p))
        return mu, float(np.dot(p, (v - mu) ** 2) / np.sum(p))
    if d[0] == "NORMAL":
        return float(d[1]), float(d[2])
    return 0.5 * (d[1] + d[2]), (d[2] - d[1]) ** 2 / 12.0


def mvnormal_lintr(name, period, positions, mean, cov) -> spStoLintr:
    """A multivariate normal N(mean, cov) over `positions` as a LINTR block: q = n standard-normal
    latents, H = the lower Cholesky factor of cov (all entries on and below the diagonal), c = mean.
    ValueError if cov is not symmetric positive definite."""
    mean = np.asarray(mean, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    n = len(positions)
    if mean.shape != (n,) or cov.shape != (n, n):
        raise ValueError(f"mvnormal_lintr: mean {mean.shape} / cov {cov.shape} do not fit {n} positions")
    if not np.isfinite(cov).all() or not np.isfinite(mean).all() or not np.array_equal(cov, cov.T):
        raise ValueError("mvnormal_lintr: cov must be finite and symmetric, mean finite")
    try:
        Lc = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise ValueError("mvnormal_lintr: cov is not positive definite") from None
    return spStoLintr(name, period, [spSmpsPosition(*p) for p in positions], [float(v) for v in mean],
                      [f"Z{l + 1}" for l in range(n)], [("NORMAL", 0.0, 1.0) for _ in range(n)],
                      [[(l, float(Lc[j, l])) for l in range(j + 1)] for j in range(n)])


def scenario_positions(sp2: spStageProblem, sto: spStoType):
    """Random-element layout for the C ABI: (positions, row[k], col[k] (-1 = RHS)).
    Row/column lookups raise KeyError like delta_coefficients (subprob.jl:112,116)."""
    rowm = {n: i for i, n in enumerate(sp2.stage_constraints)}
    colm = {n: j for j, n in enumerate(sp2.last_stage_vars)}
    positions = sto_positions(sto)
    rows = np.array([rowm[p.row_name] for p in positions], dtype=np.int32)
    cols = np.array([-1 if p.col_name in ("RHS", "rhs") else colm[p.col_name] for p in positions], dtype=np.int32)
    return positions, rows, cols


def sample_values(sto: spStoType, N: int, rng: np.random.Generator, positions=None) -> np.ndarray:
    """N i.i.d. draws of every independent element (rand(sto), smps_sto.jl:140-149):
    N x k values in `positions` order.  NORMAL uses sqrt(variance) (smps_sto.jl:122-125).
    A block draws one uniform per scenario (at its first member in `positions`), so every row holds
    one of its realisations."""
    positions = positions if positions is not None else sto_positions(sto)
    members = _block_members(sto) if sto.blocks else {}
    lmembers = _lintr_members(sto)
    picks, lvalues = {}, {}
    out = np.empty((N, len(positions)))
    for e, p in enumerate(positions):
        if p in lmembers:                 # a LINTR block draws its latents once, at its first member in `positions`
            bi, j = lmembers[p]
            if bi not in lvalues:
                b = sto.lintr[bi]
                xi = sample_values(spStoType("", dict(enumerate(b.latents))), N, rng)
                lvalues[bi] = lintr_apply(b, xi)
            out[:, e] = lvalues[bi][:, j]
            continue
        if p in members:
            bi, j = members[p]
            b = sto.blocks[bi]
            if bi not in picks:
                cdf = np.cumsum(np.asarray(b.probs, dtype=np.float64))
                u = rng.random(N) * cdf[-1]
                picks[bi] = np.minimum(np.searchsorted(cdf, u, side="right"), len(cdf) - 1)
            out[:, e] = np.asarray(b.values, dtype=np.float64)[picks[bi], j]
            continue
        d = sto.indep[p]
        if d[0] == "DISCRETE":
            vals = np.asarray(d[1], dtype=np.float64)
            cdf = np.cumsum(np.asarray(d[2], dtype=np.float64))
            u = rng.random(N) * cdf[-1]
            out[:, e] = vals[np.minimum(np.searchsorted(cdf, u, side="right"), len(vals) - 1)]
        elif d[0] == "NORMAL":
            out[:, e] = rng.normal(d[1], np.sqrt(d[2]), size=N)
        else:
            out[:, e] = rng.uniform(d[1], d[2], size=N)
    return out


def mean_values(sto: spStoType, positions=None) -> np.ndarray:
    """Mean of every element; a block member's is sum p v / sum p over the realisations, a LINTR
    member's c + sum_l h E xi_l."""
    positions = positions if positions is not None else sto_positions(sto)
    members = _block_members(sto) if sto.blocks else {}
    lmembers = _lintr_members(sto)
    out = []
    for p in positions:
        if p in lmembers:
            bi, j = lmembers[p]
            b = sto.lintr[bi]
            out.append(float(b.constants[j] + sum(h * _latent_moments(b.latents[l])[0] for l, h in b.rows[j])))
            continue
        if p in members:
            bi, j = members[p]
            b = sto.blocks[bi]
            out.append(float(np.dot(b.probs, np.asarray(b.values, dtype=np.float64)[:, j]) / np.sum(b.probs)))
            continue
        d = sto.indep[p]
        if d[0] == "DISCRETE":
            out.append(float(np.dot(d[1], d[2]) / np.sum(d[2])))
        elif d[0] == "NORMAL":
            out.append(d[1])
        else:
            out.append(0.5 * (d[1] + d[2]))
    return np.array(out)


def joint_support(sto: spStoType, positions=None, max_points=1 << 20):
    """(values[R_total, k], probs[R_total]) of an all-discrete sto: the product of the INDEP
    DISCRETE supports and the blocks' realisations, columns in `positions` order, the first factor
    (INDEP elements in file order, then the blocks, then the LINTR blocks whose latents must all be
    DISCRETE) varying slowest.  A row's probability is the
    product of its factors' probabilities as the file states them (not normalised), so
    sum(probs * f(values)) / sum(probs) is an exact expectation.  ValueError for a NORMAL or
    UNIFORM element, for a position the sto does not hold, and past max_points rows."""
    positions = positions if positions is not None else sto_positions(sto)
    index = {p: e for e, p in enumerate(positions)}
    if len(index) != len(positions):
        raise ValueError("joint_support: a position is listed twice")
    factors = []                       # (columns, values[R, n], probs[R])
    for p, d in sto.indep.items():
        if d[0] != "DISCRETE":
            raise ValueError(f"joint_support: {tuple(p)} is {d[0]}, not DISCRETE")
        factors.append(([p], np.asarray(d[1], dtype=np.float64)[:, None], np.asarray(d[2], dtype=np.float64)))
    for b in sto.blocks:
        factors.append((b.positions, np.asarray(b.values, dtype=np.float64).reshape(len(b.probs), len(b.positions)),
                        np.asarray(b.probs, dtype=np.float64)))
    for b in getattr(sto, "lintr", []):
        # the product of the latents' supports (file order, the first latent slowest), the members by lintr_apply
        for name, d in zip(b.latent_names, b.latents):
            if d[0] != "DISCRETE":
                raise ValueError(f"joint_support: latent {name} of LINTR block {b.name} is {d[0]}, not DISCRETE")
        R = 1
        for d in b.latents:
            R *= len(d[1])
            if R > max_points:
                raise ValueError(f"joint_support: more than max_points = {max_points} points")
        xi, pr, inner = np.empty((R, len(b.latents))), np.ones(R), R
        for l, d in enumerate(b.latents):
            inner //= len(d[1])
            pick = (np.arange(R) // inner) % len(d[1])
            xi[:, l] = np.asarray(d[1], dtype=np.float64)[pick]
            pr *= np.asarray(d[2], dtype=np.float64)[pick]
        factors.append((b.positions, lintr_apply(b, xi), pr))
    known = {p for f in factors for p in f[0]}
    for p in positions:
        if p not in known:
            raise ValueError(f"joint_support: {tuple(p)} is not a random element of this sto")
    factors = [f for f in factors if all(p in index for p in f[0])]
    if sum(len(f[0]) for f in factors) != len(positions):
        raise ValueError("joint_support: positions must hold whole blocks")
    total = 1
    for f in factors:
        total *= len(f[2])
        if total > max_points:
            raise ValueError(f"joint_support: more than max_points = {max_points} points")
    values = np.empty((total, len(positions)))
    probs = np.ones(total)
    inner = total
    for cols, v, p in factors:
        inner //= len(p)
        pick = (np.arange(total) // inner) % len(p)
        probs *= p[pick]
        for j, pos in enumerate(cols):
            values[:, index[pos]] = v[pick, j]
    return values, probs
