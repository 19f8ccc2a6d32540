"""Host-side mirror of the reference's TwoSD hot-path API, backed by libtwosd_hip.so.

Reference (module TwoSD, yhz0/SQLP) -> here:
  sdDualVertexSet / push!         dual_set.jl:69-127      -> sdDualVertexSet / push / .push
  sdEpigraph(prob, w, lb)         epigraph.jl:52-61       -> sdEpigraph(ctx, w, lb)
  add_scenario!(epi, w, weight)   epigraph.jl:81-96       -> add_scenario / add_scenarios
  solve_problem!(sp, x, w)        smps_routines.jl:50-62  -> solve_problem / solve_batch
  evaluate(sp1, sp2, sto, x; N)   smps_routines.jl:67-82  -> evaluate
  (none: evaluate returns the mean alone)                  -> evaluate_moments / evaluate_paired / evaluate_ci
  argmax_procedure(...)           subprob.jl:141-169      -> argmax_procedure
  build_sasa_cut(epi, x, V)       epigraph.jl:125-146     -> build_sasa_cut -> sdCut
  sd_iteration! (hot segment)     algorithm.jl:45-55,79-85 -> sd_iteration_hot_path
All arithmetic runs on the GPU through the C ABI; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _lib
from ._lib import check, ptr
from .smps import spStageProblem, spSmpsPosition, scenario_positions, sto_positions

MIN_SENSE = "MIN_SENSE"
# argmax tie rule: 0 = the reference's strict '>' (subprob.jl:156, first maximum in insertion
# order).  tie_rel > 0 is the build's near-tie rule (lowest vertex index within
# tie_rel * (1 + |max|) of the maximum), which makes the pick independent of summation order
# for scores that tie in exact arithmetic; the bench passes 1e-12 explicitly.
DEFAULT_TIE_REL = 0.0


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


@dataclass
class CanonicalForm:
    """twosd_canonical_form's output: the LP  min q'y' + c0, W y' (sense) r, y' >= 0  that the
    kernels solve for a template with general bounds, and the map back to the caller's y."""
    m_lp: int
    n_lp: int
    n_bound_rows: int
    W: tuple             # CSC (colptr, rowval, nzval), m_lp x n_lp, 0-based int64
    q: np.ndarray
    r: np.ndarray        # [r - W s ; hi - lo]
    sense: list
    c0: float
    col_src: np.ndarray  # y_j = col_off[j] + col_sign[j] * y'[col_src[j]] - y'[col_src2[j]]  (-1: no term)
    col_sign: np.ndarray
    col_off: np.ndarray
    col_src2: np.ndarray
    box_col: np.ndarray  # column of bound row m2 + b

    def map_back(self, y_lp) -> np.ndarray:
        """LP solution(s) (.. x n_lp) -> the caller's y (.. x n2)."""
        y_lp = np.asarray(y_lp, dtype=np.float64)
        ext = np.concatenate([y_lp, np.zeros(y_lp.shape[:-1] + (1,))], axis=-1)   # index -1 reads the zero
        return self.col_off + self.col_sign * ext[..., self.col_src] - ext[..., self.col_src2]


def canonical_form(W, q, r, sense, ylb=None, yub=None) -> CanonicalForm:
    """twosd_canonical_form (host code of the library, no GPU): W is a CSC triple (colptr, rowval,
    nzval), 0-based; ylb / yub default to 0 / +inf.  Raises TwoSDError(TWOSD_E_ARG) for bounds that
    are no interval."""
    lib = _lib.load()
    cp, rv, nz = (np.ascontiguousarray(W[0], dtype=np.int64), np.ascontiguousarray(W[1], dtype=np.int64), _f64(W[2]))
    q, r = _f64(q), _f64(r)
    m2, n2, nnz = len(r), len(q), len(nz)
    sb = np.frombuffer("".join(sense).encode(), dtype=np.int8).copy()
    lo = None if ylb is None else _f64(ylb)
    hi = None if yub is None else _f64(yub)
    m_lp, n_lp, nb = C.c_int(), C.c_int(), C.c_int()
    ocp = np.zeros(2 * n2 + 1, dtype=np.int64)
    orv = np.zeros(2 * nnz + n2, dtype=np.int64)
    onz = np.zeros(2 * nnz + n2)
    oq = np.zeros(2 * n2)
    orr = np.zeros(m2 + n2)
    osn = np.zeros(m2 + n2, dtype=np.int8)
    c0 = C.c_double()
    src = np.zeros(n2, dtype=np.int32)
    src2 = np.zeros(n2, dtype=np.int32)
    sign = np.zeros(n2)
    off = np.zeros(n2)
    box = np.zeros(n2, dtype=np.int32)
    check(lib.twosd_canonical_form(m2, n2, ptr(cp), ptr(rv), ptr(nz), ptr(q), ptr(r), ptr(sb), ptr(lo), ptr(hi), 0,
                                   C.byref(m_lp), C.byref(n_lp), C.byref(nb), ptr(ocp), ptr(orv), ptr(onz), ptr(oq),
                                   ptr(orr), ptr(osn), C.byref(c0), ptr(src), ptr(sign), ptr(off), ptr(src2), ptr(box)))
    ml, nl = m_lp.value, n_lp.value
    nnz_lp = int(ocp[nl])
    return CanonicalForm(ml, nl, nb.value, (ocp[:nl + 1].copy(), orv[:nnz_lp].copy(), onz[:nnz_lp].copy()), oq[:nl].copy(),
                         orr[:ml].copy(), [chr(v) for v in osn[:ml]], c0.value, src, sign, off, src2, box[:nb.value].copy())


@dataclass
class sdCut:
    """eta >= alpha + beta'x (epigraph.jl:5-12); never scaled.  picks: the handle of the argmax
    picks the cut was built with (twosd_picks_keep; build_sasa_cut(keep_picks=True)), or None."""
    alpha: float
    beta: np.ndarray
    weight_mark: float
    picks: Optional[int] = None


class SDContext:
    """Device-resident hot-path state of one cell on one GPU: the stage-2 template
    (extract_coefficients, subprob.jl:15-69), the random-element layout, the shared
    warm-start basis, and the dual vertex set (cell.dual_vertices, cell.jl:25)."""

    def __init__(self, sp2: spStageProblem, sto=None, positions=None, device: int = 0, index_base: int = 0):
        """index_base = 1 hands the template and positions to the library 1-based, as a Julia
        caller passes SparseMatrixCSC colptr / rowval (twosd_set_template, index_base)."""
        self.lib = _lib.load()
        self.index_base = int(index_base)
        h = C.c_void_p()
        check(self.lib.twosd_create(device, C.byref(h)))
        self.h = h
        self._set_problem(sp2, sto, positions)

    def _set_problem(self, sp2: spStageProblem, sto=None, positions=None):
        """Template and random-element layout of this handle (twosd_set_template clears the
        basis, scenarios, dual vertex set and cuts of an earlier one)."""
        self.sp2 = sp2
        self.m, self.n1, self.n2 = sp2.shape
        Tcp, Trv, Tnz = sp2.T
        Wcp, Wrv, Wnz = sp2.W
        ib = self.index_base
        self._keep = [np.ascontiguousarray(a + ib if a.dtype.kind == "i" else a)
                      for a in (Tcp, Trv, Tnz, Wcp, Wrv, Wnz)]
        sense = np.frombuffer("".join(sp2.sense).encode(), dtype=np.int8).copy()
        self._keep += [sense]
        check(self.lib.twosd_set_template(
            self.h, self.m, self.n1, self.n2,
            ptr(self._keep[0]), ptr(self._keep[1]), ptr(self._keep[2]),
            ptr(self._keep[3]), ptr(self._keep[4]), ptr(self._keep[5]),
            ptr(_f64(sp2.q)), ptr(_f64(sp2.r)), ptr(sense), ptr(_f64(sp2.ylb)), ptr(_f64(sp2.yub)), ib))
        # the LP the kernels solve (twosd_lp_shape): general bounds cost one row per boxed variable.
        # mv = m_lp = m + n_bound_rows is the length of a dual vector (row duals, then the boxed
        # variables' multipliers) and of a basis head; all equal m / n2 with default bounds.
        ml, nl, nb = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.twosd_lp_shape(self.h, C.byref(ml), C.byref(nl), C.byref(nb)))
        self.m_lp, self.n_lp, self.n_bound_rows = ml.value, nl.value, nb.value
        self.mv = self.m_lp
        self.row_lookup = {n: i for i, n in enumerate(sp2.stage_constraints)}
        self.col_lookup = {n: j for j, n in enumerate(sp2.last_stage_vars)}
        if sto is not None and positions is None:
            positions = sto_positions(sto)
        self.set_positions(positions or [])
        self.has_basis = False

    def set_positions(self, positions):
        """Random-element layout; KeyError for an unknown row/column like
        delta_coefficients (subprob.jl:112,116); ValueError, before any device call, for an element
        listed twice (the reference keeps the last write, subprob.jl:114-117; the kernels would add
        both deltas, so twosd_set_random_positions refuses it too).  The order of the listing fixes
        the columns of the value arrays only: every decision uses the canonical element order
        (ascending row, RHS first, then T columns ascending)."""
        new = [spSmpsPosition(*p) for p in positions]
        rows = np.array([self.row_lookup[p.row_name] for p in new], dtype=np.int32)
        cols = np.array([-1 if p.col_name in ("RHS", "rhs") else self.col_lookup[p.col_name]
                         for p in new], dtype=np.int32)
        seen = {}
        for e, rc in enumerate(zip(rows.tolist(), cols.tolist())):
            if rc in seen:
                raise ValueError(f"positions {seen[rc]} and {e} are the same element {tuple(new[e])}")
            seen[rc] = e
        self.positions = new
        self.pos_index = {p: e for e, p in enumerate(self.positions)}
        self.k = len(self.positions)
        self.rows, self.cols = rows, cols
        ib = self.index_base
        rows_b = np.ascontiguousarray(rows + ib, dtype=np.int32)
        cols_b = np.ascontiguousarray(np.where(cols < 0, -1, cols + ib), dtype=np.int32)
        check(self.lib.twosd_set_random_positions(self.h, self.k, ptr(rows_b), ptr(cols_b), ib))
        # template value of every element (for scenario -> values conversion)
        T = self.sp2.dense_T()
        self.template_values = np.array(
            [self.sp2.r[r] if c < 0 else T[r, c] for r, c in zip(rows, cols)], dtype=np.float64)

    def close(self):
        if getattr(self, "h", None):
            self.lib.twosd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- warm-start basis -------------------------------------------------------
    def compute_basis(self, x, values=None):
        """Optimal basis of the scenario `values` (default: template) at x, installed as the
        shared warm start of every scenario solve."""
        x = _f64(x)
        v = None if values is None else _f64(values)
        check(self.lib.twosd_compute_basis(self.h, ptr(x), ptr(v)))
        self.has_basis = True

    def set_basis(self, head):
        head = np.ascontiguousarray(head, dtype=np.int32)
        check(self.lib.twosd_set_basis(self.h, ptr(head)))
        self.has_basis = True

    def get_basis(self):
        head = np.zeros(self.m_lp, dtype=np.int32)
        check(self.lib.twosd_get_basis(self.h, ptr(head)))
        return head

    # -- warm-start basis pool (twosd_pool_*: fewer pivots, identical vertices) ---
    def pool_add_basis(self, head) -> bool:
        head = np.ascontiguousarray(head, dtype=np.int32)
        added = C.c_int(0)
        check(self.lib.twosd_pool_add_basis(self.h, ptr(head), C.byref(added)))
        return bool(added.value)

    def pool_build(self, epi, x, first, count, max_pool) -> int:
        """Add the most frequent optimal bases of scenarios [first, first+count) of `epi`
        at x to the pool (up to max_pool bases); returns the pool size."""
        x = _f64(x)
        n = C.c_int(0)
        check(self.lib.twosd_pool_build(self.h, epi.index, ptr(x), int(first), int(count), int(max_pool),
                                        C.byref(n)))
        return n.value

    def pool_build_candidates(self, epi, x, first, count, level1, ncand):
        """Two-level warm-start selection: level 1 over the first `level1` pool bases, level 2
        over the `ncand` bases a flat selection picks most often for the training scenarios
        [first, first+count) of `epi` that share the level-1 pick.  level1 = 0: flat."""
        check(self.lib.twosd_pool_build_candidates(self.h, epi.index, ptr(_f64(x)), int(first), int(count),
                                                   int(level1), int(ncand)))

    def last_pool_picks(self, N):
        """Pool basis every scenario of the last LP batch started from."""
        picks = np.zeros(N, dtype=np.int32)
        check(self.lib.twosd_last_pool_picks(self.h, int(N), ptr(picks)))
        return picks

    def invalidate_x(self):
        """Drop the per-x cache (next solve / cut recomputes it; results unchanged)."""
        check(self.lib.twosd_invalidate_x(self.h))

    def pool_refresh(self, epi, x, first, count, max_pool) -> int:
        """Replace the warm-start pool by the primary basis plus the max_pool - 1 most frequent
        optimal bases of training scenarios [first, first+count) of epi at x (twosd_pool_refresh)."""
        n = C.c_int()
        check(self.lib.twosd_pool_refresh(self.h, epi.index, ptr(_f64(x)), first, count, max_pool, C.byref(n)))
        return n.value

    # -- distributed refresh (twosd_refresh_*; driven by sqlp_amd.dist.refresh_sharded) --------
    def refresh_train(self, epi, x, first, count):
        """Training solves of this rank's slice; returns (keys u64, counts, first scenarios, box
        lo, box hi) of its distinct optimal bases."""
        U = C.c_int()
        lo = np.zeros(max(self.k, 1))
        hi = np.zeros(max(self.k, 1))
        check(self.lib.twosd_refresh_train(self.h, epi.index, ptr(_f64(x)), int(first), int(count), C.byref(U),
                                           ptr(lo), ptr(hi)))
        keys = np.zeros(U.value, dtype=np.uint64)
        counts = np.zeros(U.value, dtype=np.int32)
        reps = np.zeros(U.value, dtype=np.int32)
        check(self.lib.twosd_refresh_train_bases(self.h, ptr(keys), ptr(counts), ptr(reps)))
        return keys, counts, reps, lo[:self.k], hi[:self.k]

    def refresh_train_ex(self, epi, x, first, count, kcap):
        """Training solves of this rank's slice under the pivot cap kcap (> 0; <= 0 none), one
        launch, no retry (twosd_refresh_train_ex); returns (keys u64, counts, first scenarios,
        box lo, box hi, optimal training scenarios)."""
        U = C.c_int()
        nopt = C.c_int()
        lo = np.zeros(max(self.k, 1))
        hi = np.zeros(max(self.k, 1))
        check(self.lib.twosd_refresh_train_ex(self.h, epi.index, ptr(_f64(x)), int(first), int(count), int(kcap),
                                              C.byref(U), C.byref(nopt), ptr(lo), ptr(hi)))
        keys = np.zeros(U.value, dtype=np.uint64)
        counts = np.zeros(U.value, dtype=np.int32)
        reps = np.zeros(U.value, dtype=np.int32)
        check(self.lib.twosd_refresh_train_bases(self.h, ptr(keys), ptr(counts), ptr(reps)))
        return keys, counts, reps, lo[:self.k], hi[:self.k], nopt.value

    def refresh_cap_stats(self):
        """(pivot sum, scenarios) of the last LP batch of >= 4096 scenarios: the scale of the
        training pivot cap (twosd_refresh_cap_stats)."""
        s = C.c_int64()
        n = C.c_int64()
        check(self.lib.twosd_refresh_cap_stats(self.h, C.byref(s), C.byref(n)))
        return s.value, n.value

    def cut_stats(self):
        """(scenarios re-decided in the restatement's arithmetic, candidates scored, full
        re-scans, dominated twin vertices left out) of the last cut (twosd_cut_stats)."""
        out = np.zeros(4, dtype=np.int64)
        check(self.lib.twosd_cut_stats(self.h, ptr(out)))
        return tuple(int(v) for v in out)

    def cut_pass(self):
        """(fp32, band) of the last cut: 1 if its MFMA pass ran in fp32, 0 for fp64, and that
        pass's decision band (twosd_cut_pass)."""
        f = C.c_int()
        b = C.c_double()
        check(self.lib.twosd_cut_pass(self.h, C.byref(f), C.byref(b)))
        return f.value, b.value

    def cut_pass_kind(self):
        """(kind, limbs, pairs) of the last cut: kind 0 the fp64 MFMA pass, 1 the fp32 one, 2 the
        integer (int8-limb) one; the integer pass's limb count and kept limb pairs
        (twosd_cut_pass_kind)."""
        kind, limbs, pairs = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.twosd_cut_pass_kind(self.h, C.byref(kind), C.byref(limbs), C.byref(pairs)))
        return kind.value, limbs.value, pairs.value

    def cut_debug_scores(self, epi, x, n, nv):
        """The integer pass's fp32 score terms of one cut of epigraph `epi` (n scenarios, nv
        vertices) at x: (t[n, nvc], vmap[nvc]) over the compacted vertices (twosd_cut_debug_scores)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros(n * nv, dtype=np.float32)
        vmap = np.zeros(nv, dtype=np.int32)
        nvc = C.c_int()
        check(self.lib.twosd_cut_debug_scores(self.h, int(epi), ptr(x), ptr(out), out.size, C.byref(nvc), ptr(vmap)))
        return out[:n * nvc.value].reshape(n, nvc.value).copy(), vmap[:nvc.value].copy()

    def training_cap(self, pivots_sum, scenarios) -> int:
        """The refresh's training pivot cap for a last large batch of `scenarios` solves with
        `pivots_sum` pivots (twosd_training_cap: the native rule, this context's setting)."""
        cap = C.c_int()
        check(self.lib.twosd_training_cap(self.h, int(pivots_sum), int(scenarios), C.byref(cap)))
        return cap.value

    def last_objective(self):
        """(sum_s w_s obj_s, sum_s w_s) of the last solve_batch / solve_push / solve_values batch
        (twosd_last_objective): the incumbent objective at x is their quotient."""
        a = C.c_double()
        b = C.c_double()
        check(self.lib.twosd_last_objective(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def refresh_build_local(self, reps) -> int:
        """Compose the bases this rank owns (first scenarios `reps`, selection order); returns the
        pack size in bytes."""
        reps = np.ascontiguousarray(reps, dtype=np.int32)
        nb = C.c_int64()
        check(self.lib.twosd_refresh_build_local(self.h, len(reps), ptr(reps), C.byref(nb)))
        return nb.value

    def refresh_pack(self, d_dst: int):
        check(self.lib.twosd_refresh_pack(self.h, C.c_void_p(d_dst)))

    def refresh_assemble(self, G, d_packs: int, stride: int, order, box_lo, box_hi) -> int:
        order = np.ascontiguousarray(order, dtype=np.int32)
        n = C.c_int()
        check(self.lib.twosd_refresh_assemble(self.h, int(G), C.c_void_p(d_packs), C.c_int64(stride), len(order),
                                              ptr(order), ptr(_f64(box_lo)), ptr(_f64(box_hi)), C.byref(n)))
        return n.value

    def pool_candidate_picks(self, epi, x, first, count, level1):
        p1 = np.zeros(count, dtype=np.int32)
        pf = np.zeros(count, dtype=np.int32)
        check(self.lib.twosd_pool_candidate_picks(self.h, epi.index, ptr(_f64(x)), int(first), int(count), int(level1),
                                                  ptr(p1), ptr(pf)))
        return p1, pf

    def pool_set_candidates(self, level1, ncand, p1, pf):
        p1 = np.ascontiguousarray(p1, dtype=np.int32)
        pf = np.ascontiguousarray(pf, dtype=np.int32)
        check(self.lib.twosd_pool_set_candidates(self.h, int(level1), int(ncand), len(p1), ptr(p1), ptr(pf)))

    def set_refresh_kcap(self, kcap: int):
        """Pivot cap of the refresh's training solves: > 0 explicit, 0 auto (3 x the mean pivots of
        the last batch of >= 4096 scenarios, at least 32), < 0 none (the kernel's kmax)."""
        check(self.lib.twosd_set_refresh_kcap(self.h, int(kcap)))
        self.refresh_kcap = int(kcap)

    def last_lp_iters(self, N):
        """(pivots, status) of the first N scenarios of the last LP launch."""
        it = np.zeros(N, dtype=np.int32)
        st = np.zeros(N, dtype=np.int32)
        check(self.lib.twosd_last_lp_iters(self.h, int(N), ptr(it), ptr(st)))
        return it, st

    def last_refresh_ms(self):
        """[training solves, re-solves, host composition, upload, total] of the last refresh."""
        out = np.zeros(5)
        check(self.lib.twosd_last_refresh_ms(self.h, ptr(out)))
        return out

    def pool_size(self) -> int:
        n = C.c_int(0)
        check(self.lib.twosd_pool_size(self.h, C.byref(n)))
        return n.value

    def pool_get(self, p):
        head = np.zeros(self.m_lp, dtype=np.int32)
        check(self.lib.twosd_pool_get(self.h, int(p), ptr(head)))
        return head

    # -- on-device scenario sampler (rand(rng, sto), smps_sto.jl:117-149) ----------
    def set_distributions(self, sto):
        """Upload the distribution of every random element (position order): the independent ones,
        and the joint discrete blocks of sto.blocks (twosd_set_distributions_joint; every member of
        a block must be a position of this context), and the LINTR blocks of sto.lintr
        (twosd_set_distributions_lintr: members affine in a few independent latent variables)."""
        blocks = getattr(sto, "blocks", [])
        lintr = getattr(sto, "lintr", [])
        member = {p for b in blocks for p in b.positions}
        lmember = {p for b in lintr for p in b.positions}
        kinds, nsup, vals, probs, p0, p1 = [], [], [], [], [], []
        for pos in self.positions:
            if pos in lmember:
                kinds.append(_lib.DIST_LINTR); nsup.append(0); p0.append(0.0); p1.append(0.0)
                continue
            if pos in member:
                kinds.append(_lib.DIST_BLOCK); nsup.append(0); p0.append(0.0); p1.append(0.0)
                continue
            d = sto.indep[pos]
            if d[0] == "DISCRETE":
                kinds.append(0); nsup.append(len(d[1])); vals += list(d[1]); probs += list(d[2])
                p0.append(0.0); p1.append(0.0)
            elif d[0] == "NORMAL":
                kinds.append(1); nsup.append(0); p0.append(d[1]); p1.append(d[2])
            else:
                kinds.append(2); nsup.append(0); p0.append(d[1]); p1.append(d[2])
        a = [np.ascontiguousarray(kinds, dtype=np.int32), np.ascontiguousarray(nsup, dtype=np.int32),
             _f64(vals if vals else [0.0]), _f64(probs if probs else [0.0]), _f64(p0), _f64(p1)]
        if not blocks and not lintr:
            check(self.lib.twosd_set_distributions(self.h, self.k, *[ptr(v) for v in a]))
            return
        moff, mem, nreal, bp, bv = [0], [], [], [], []
        for b in blocks:
            mem += [self.pos_index[p] for p in b.positions]
            moff.append(len(mem))
            nreal.append(len(b.probs))
            bp += list(b.probs)
            bv += list(np.asarray(b.values, dtype=np.float64).reshape(len(b.probs), len(b.positions)).ravel())
        j = [np.ascontiguousarray(moff, dtype=np.int32), np.ascontiguousarray(mem, dtype=np.int32),
             np.ascontiguousarray(nreal, dtype=np.int32), _f64(bp if bp else [0.0]), _f64(bv if bv else [0.0])]
        if not lintr:
            check(self.lib.twosd_set_distributions_joint(self.h, self.k, *[ptr(v) for v in a], len(blocks), *[ptr(v) for v in j]))
            return
        # LINTR blocks (twosd_set_distributions_lintr): members and constants, the latents as
        # set_distributions reads an element, one CSR over the member rows
        i32 = lambda v: np.ascontiguousarray(v if len(v) else [0], dtype=np.int32)
        lmoff, lmem, lc, loff, lk, lns, lv, lp, l0, l1, rptr, col, val = [0], [], [], [0], [], [], [], [], [], [], [0], [], []
        for b in lintr:
            lmem += [self.pos_index[p] for p in b.positions]
            lc += [float(v) for v in b.constants]
            lmoff.append(len(lmem))
            for d in b.latents:
                if d[0] == "DISCRETE":
                    lk.append(0); lns.append(len(d[1])); lv += list(d[1]); lp += list(d[2]); l0.append(0.0); l1.append(0.0)
                else:
                    lk.append(1 if d[0] == "NORMAL" else 2); lns.append(0); l0.append(d[1]); l1.append(d[2])
            loff.append(len(lk))
            for row in b.rows:
                col += [l for l, _ in row]
                val += [h for _, h in row]
                rptr.append(len(col))
        keep = [i32(lmoff), i32(lmem), _f64(lc), i32(loff), i32(lk), i32(lns), _f64(lv if lv else [0.0]), _f64(lp if lp else [0.0]),
                _f64(l0), _f64(l1), i32(rptr), i32(col), _f64(val if val else [0.0])]
        L = _lib.Lintr(len(lintr), *[ptr(v) for v in keep])
        check(self.lib.twosd_set_distributions_lintr(self.h, self.k, *[ptr(v) for v in a], len(blocks), *[ptr(v) for v in j],
                                                     C.byref(L)))

    def scenario_values(self, scenario) -> np.ndarray:
        """spSmpsScenario (list of position => value) -> value vector in layout order.
        Elements a scenario omits keep their template value (delta 0)."""
        v = self.template_values.copy()
        for pos, val in scenario:
            pos = spSmpsPosition(*pos)
            if pos not in self.pos_index:
                # unknown position: KeyError on its row / column like subprob.jl:112,116
                self.row_lookup[pos.row_name]
                if pos.col_name not in ("RHS", "rhs"):
                    self.col_lookup[pos.col_name]
                raise KeyError(f"{pos} is not a random element of this context")
            v[self.pos_index[pos]] = val
        return v

    def timings_us(self):
        """[LP kernel, dedup, cut partial, cut finalize, pool selection] of the last calls."""
        t = np.zeros(5)
        check(self.lib.twosd_last_timings(self.h, ptr(t)))
        return t

    def lp_stats(self):
        s = C.c_int64()
        mx = C.c_int()
        check(self.lib.twosd_last_lp_stats(self.h, C.byref(s), C.byref(mx)))
        return s.value, mx.value

    def lp_eta_entries(self) -> int:
        """Eta-arena entries (12 B each) the last LP batch wrote (twosd_last_lp_eta_entries)."""
        return self.lp_counts()[0]

    def lp_counts(self):
        """(eta-arena entries, pool starts retried from the primary basis) of the last LP batch."""
        e = C.c_int64()
        r = C.c_int64()
        check(self.lib.twosd_last_lp_eta_entries(self.h, C.byref(e), C.byref(r)))
        return e.value, r.value

    def last_push_reps(self) -> int:
        """Scenarios whose dual the last solve_push recovered and pushed (first scenario of
        each distinct optimal dual vertex of the batch)."""
        r = C.c_int()
        check(self.lib.twosd_last_push_reps(self.h, C.byref(r)))
        return r.value

    def last_push_mode(self) -> int:
        """1 if the last solve_push recovered every dual in its main pass (full mode), 0 if it
        re-solved the representatives (twosd_last_push_mode)."""
        r = C.c_int()
        check(self.lib.twosd_last_push_mode(self.h, C.byref(r)))
        return r.value

    def lp_flops(self):
        """Counted fp64 FLOPs of the last LP batch (2 * row width per executed row op)."""
        ops = C.c_int64()
        w = C.c_int()
        check(self.lib.twosd_last_lp_ops(self.h, C.byref(ops), C.byref(w)))
        return 2.0 * w.value * ops.value

    # -- multi-GPU split of build_sasa_cut (device buffers from the caller) --------
    def cut_partial_len(self):
        a = C.c_int64()
        b = C.c_int64()
        check(self.lib.twosd_cut_partial_len(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def cut_partial(self, epi, x, tie_rel, total_weight, d_hist_ptr, d_sums_ptr):
        check(self.lib.twosd_cut_partial(self.h, epi.index, ptr(_f64(x)), float(tie_rel), float(total_weight),
                                         C.c_void_p(d_hist_ptr), C.c_void_p(d_sums_ptr), None, None))

    def cut_finalize(self, x, d_hist_ptr, d_sums_ptr):
        a = C.c_double()
        beta = np.zeros(self.n1)
        check(self.lib.twosd_cut_finalize(self.h, ptr(_f64(x)), C.c_void_p(d_hist_ptr), C.c_void_p(d_sums_ptr),
                                          C.byref(a), ptr(beta)))
        return a.value, beta

    # -- solve_problem! / evaluate ----------------------------------------------
    def solve_values(self, x, values, want_pi=True, want_y=False, raise_on_status=True):
        values = _f64(np.atleast_2d(values))
        N = values.shape[0]
        obj = np.zeros(N)
        st = np.zeros(N, dtype=np.int32)
        pi = np.zeros((N, self.mv)) if want_pi else None
        y = np.zeros((N, self.n2)) if want_y else None
        rc = self.lib.twosd_solve_values(self.h, ptr(_f64(x)), N, ptr(values), ptr(obj), ptr(pi), ptr(y), ptr(st))
        if rc != 0 and not (rc == -4 and not raise_on_status):
            check(rc)
        return obj, y, pi, st


class sdDualVertexSet:
    """Device-resident dual vertex set of an SDContext (dual_set.jl:69-127).  There is one
    set per context (the cell's shared set)."""

    def __init__(self, ctx: SDContext, data=None):
        self.ctx = ctx
        if data is not None:
            self.push_batch(np.atleast_2d(np.asarray(data, dtype=np.float64)))

    def push(self, vec):
        """push!(dvs, vec): appends iff no equal vertex exists; returns self (dual_set.jl:84-94)."""
        self.push_batch(np.asarray(vec, dtype=np.float64)[None, :])
        return self

    def push_batch(self, pis) -> np.ndarray:
        """Sequential push! of every row; returns the vertex index of each row."""
        pis = _f64(np.atleast_2d(pis))
        if pis.shape[1] != self.ctx.mv:
            raise ValueError(f"dual vector length {pis.shape[1]} != {self.ctx.mv}")
        out = np.zeros(pis.shape[0], dtype=np.int32)
        ns = C.c_int()
        check(self.ctx.lib.twosd_dvs_push(self.ctx.h, pis.shape[0], ptr(pis), ptr(out), C.byref(ns)))
        return out

    def __len__(self):
        s = C.c_int()
        check(self.ctx.lib.twosd_dvs_size(self.ctx.h, C.byref(s)))
        return s.value

    def matrix(self, first=0, count=None) -> np.ndarray:
        n = len(self)
        count = n - first if count is None else count
        out = np.zeros((count, self.ctx.mv))
        check(self.ctx.lib.twosd_dvs_get(self.ctx.h, first, count, ptr(out)))
        return out

    def __iter__(self):
        return iter(list(self.matrix()))

    def clear(self):
        check(self.ctx.lib.twosd_dvs_clear(self.ctx.h))

    def truncate(self, size):
        check(self.ctx.lib.twosd_dvs_truncate(self.ctx.h, int(size)))

    def fingerprint(self) -> int:
        """Order-dependent 64-bit digest of the set (twosd_dvs_fingerprint)."""
        d = C.c_uint64()
        check(self.ctx.lib.twosd_dvs_fingerprint(self.ctx.h, C.byref(d)))
        return d.value


def push(dvs: sdDualVertexSet, vec):
    return dvs.push(vec)


def fray_key(ray):
    """(key, normalised ray) of one feasibility ray: what a push into sdFeasRaySet computes
    (twosd_fray_key: a pure host function).  An all-zero or non-finite ray raises."""
    ray = _f64(ray).ravel()
    key = C.c_uint64()
    out = np.zeros(ray.shape[0])
    check(_lib.load().twosd_fray_key(ptr(ray), ray.shape[0], C.byref(key), ptr(out)))
    return key.value, out


class sdFeasRaySet:
    """Device-resident set F of normalised feasibility rays of an SDContext.
    There is one set per context; twosd_set_template and set_positions drop it."""

    def __init__(self, ctx: SDContext):
        self.ctx = ctx

    def push_batch(self, rays) -> np.ndarray:
        """Push every row in order; returns the index each row maps to (first occurrence kept)."""
        rays = _f64(np.atleast_2d(rays))
        if rays.shape[1] != self.ctx.mv:
            raise ValueError(f"ray length {rays.shape[1]} != {self.ctx.mv}")
        out = np.zeros(rays.shape[0], dtype=np.int32)
        ns = C.c_int()
        check(self.ctx.lib.twosd_fray_push(self.ctx.h, rays.shape[0], ptr(rays), ptr(out), C.byref(ns)))
        return out

    @property
    def size(self) -> int:
        s = C.c_int()
        check(self.ctx.lib.twosd_fray_size(self.ctx.h, C.byref(s)))
        return s.value

    def __len__(self):
        return self.size

    def get(self, first=0, count=None) -> np.ndarray:
        count = self.size - first if count is None else count
        out = np.zeros((count, self.ctx.mv))
        check(self.ctx.lib.twosd_fray_get(self.ctx.h, int(first), int(count), ptr(out)))
        return out

    def clear(self):
        check(self.ctx.lib.twosd_fray_clear(self.ctx.h))


@dataclass
class RayBatch:
    """Result of solve_rays: the infeasible scenarios' count, and per returned ray its scenario
    (index of the epigraph), the raw ray sigma = +-e_r' B^{-1}, the leaving row r and the basis head
    at the exit; status of every scenario of the batch."""
    n_infeasible: int
    scen: np.ndarray
    rays: np.ndarray
    row: np.ndarray
    head: np.ndarray
    status: np.ndarray


def solve_rays(epi: "sdEpigraph", x, first=0, count=None, cap=256, push=True) -> RayBatch:
    """Solve scenarios [first, first+count) of epi at x and recover one Farkas ray per distinct
    infeasible exit (twosd_solve_rays), at most cap, in scenario order; push=True also pushes them
    into the context's sdFeasRaySet on the device.  Infeasible scenarios do not raise; a scenario
    that ends at the iteration limit or numerically does."""
    ctx = epi.ctx
    count = epi.num_scenarios - first if count is None else count
    cap = int(cap)
    scen = np.zeros(max(cap, 1), dtype=np.int32)
    rays = np.zeros((max(cap, 1), ctx.mv))
    row = np.zeros(max(cap, 1), dtype=np.int32)
    head = np.zeros((max(cap, 1), ctx.mv), dtype=np.int32)
    st = np.zeros(max(count, 1), dtype=np.int32)
    ni, nr = C.c_int(), C.c_int()
    check(ctx.lib.twosd_solve_rays(ctx.h, epi.index, ptr(_f64(x)), int(first), int(count), cap, 1 if push else 0,
                                   C.byref(ni), C.byref(nr), ptr(scen), ptr(rays), ptr(row), ptr(head), ptr(st)))
    n = nr.value
    return RayBatch(ni.value, scen[:n], rays[:n], row[:n], head[:n], st[:count])


def last_ray_stats(ctx: SDContext):
    """(list positions re-solved, infeasible scenarios the scan filter dropped) of the last solve_rays."""
    a, b = C.c_int64(), C.c_int64()
    check(ctx.lib.twosd_last_ray_stats(ctx.h, C.byref(a), C.byref(b), None))
    return a.value, b.value


def last_scan_us(ctx: SDContext) -> float:
    """Device time (events) of the scan and merge kernels of the last feas_scan, in microseconds."""
    t = C.c_double()
    check(ctx.lib.twosd_last_ray_stats(ctx.h, None, None, C.byref(t)))
    return t.value


@dataclass
class FeasScan:
    """Result of feas_scan: per ray of F its largest score over the scenarios and the lowest
    scenario attaining it, the feasibility row alpha + beta'x <= 0 of that pair, and per scenario
    whether any ray cuts it off at x (score > 0)."""
    ray_max: np.ndarray
    ray_arg: np.ndarray
    alpha: np.ndarray
    beta: np.ndarray
    n_cut_off: int
    cut_off: np.ndarray


def feas_scan(epi: "sdEpigraph", x, first=0, count=None) -> FeasScan:
    """Violation scan of scenarios [first, first+count) of epi against every ray of the context's
    sdFeasRaySet at x (twosd_feas_scan).  An empty ray set raises (TWOSD_E_STATE)."""
    ctx = epi.ctx
    count = epi.num_scenarios - first if count is None else count
    s = C.c_int()
    check(ctx.lib.twosd_fray_size(ctx.h, C.byref(s)))
    J = max(s.value, 1)
    rmax = np.zeros(J)
    rarg = np.zeros(J, dtype=np.int32)
    alpha = np.zeros(J)
    beta = np.zeros((J, ctx.n1))
    ncut = C.c_int64()
    cut = np.zeros(max(count, 1), dtype=np.uint8)
    check(ctx.lib.twosd_feas_scan(ctx.h, epi.index, ptr(_f64(x)), int(first), int(count), ptr(rmax), ptr(rarg), ptr(alpha),
                                  ptr(beta), C.byref(ncut), ptr(cut)))
    return FeasScan(rmax, rarg, alpha, beta, ncut.value, cut[:count].astype(bool))


class sdEpigraph:
    """sdEpigraph (epigraph.jl:17-61): scenario pool + weights on the device, cuts on the host."""

    def __init__(self, ctx: SDContext, objective_weight: float, lower_bound: float):
        self.ctx = ctx
        self.objective_weight = float(objective_weight)
        self.lower_bound = float(lower_bound)
        e = C.c_int()
        check(ctx.lib.twosd_epigraph_create(ctx.h, C.byref(e)))
        self.index = e.value
        self.scenario_weight: list = []
        self.cuts: list = []
        self.incumbent_cut = None
        self._pick_handles: set = set()   # live pick handles kept for this epigraph's cuts

    @property
    def total_scenario_weight(self) -> float:
        tw = C.c_double()
        check(self.ctx.lib.twosd_epigraph_info(self.ctx.h, self.index, None, C.byref(tw)))
        return tw.value

    @property
    def num_scenarios(self) -> int:
        n = C.c_int()
        check(self.ctx.lib.twosd_epigraph_info(self.ctx.h, self.index, C.byref(n), None))
        return n.value


def add_scenario(epi: sdEpigraph, scenario, weight: float = 1.0):
    """add_scenario!(epi, scenario, weight) (epigraph.jl:81-96)."""
    add_scenarios(epi, epi.ctx.scenario_values(scenario)[None, :], np.array([weight]))


def add_scenarios(epi: sdEpigraph, values, weights=None):
    """Batched add_scenario!: values N x k (layout order), weights N (default 1.0)."""
    values = _f64(np.atleast_2d(values))
    N = values.shape[0]
    w = None if weights is None else _f64(weights)
    check(epi.ctx.lib.twosd_add_scenarios(epi.ctx.h, epi.index, N, ptr(values), ptr(w)))
    epi.scenario_weight.extend([1.0] * N if w is None else list(w))


@dataclass(frozen=True)
class Sampling:
    """struct twosd_sampling: how a device-drawn stream is built.  Groups of `group` consecutive
    global scenario indices are dependent (antithetic pairs, Latin hypercube blocks of S), so the
    estimators that take a plan report moments over group means.  sampling=None means i.i.d."""
    mode: int = _lib.SAMPLING_IID
    group: int = 1

    @classmethod
    def iid(cls) -> "Sampling":
        return cls(_lib.SAMPLING_IID, 1)

    @classmethod
    def antithetic(cls) -> "Sampling":
        return cls(_lib.SAMPLING_ANTITHETIC, 2)

    @classmethod
    def lhs(cls, S) -> "Sampling":
        """Latin hypercube blocks of S scenarios, 2 <= S <= 256 (the library checks)."""
        return cls(_lib.SAMPLING_LHS, int(S))

    def _c(self):
        return _lib.SamplingPlan(int(self.mode), int(self.group))


def _plan(sampling):
    """(pointer or None, group) of a sampling= argument; the struct must outlive the call, so the
    caller keeps the returned object."""
    if sampling is None:
        return None, 1
    return sampling._c(), int(sampling.group)


def add_sampled_scenarios(epi: sdEpigraph, N, seed, first_index=0, weights=None, sampling=None):
    """N scenarios drawn on the device (Philox4x32-10 stream (seed, first_index + s, e))
    appended to epi -- add_scenario!(epi, rand(rng, sto)) N times without a host copy.
    sampling: a Sampling plan (twosd_add_sampled_scenarios_vr); first_index and N are then whole
    groups."""
    w = None if weights is None else _f64(weights)
    if sampling is None:
        check(epi.ctx.lib.twosd_add_sampled_scenarios(epi.ctx.h, epi.index, int(N), C.c_uint64(seed),
                                                       C.c_uint64(first_index), ptr(w)))
    else:
        plan, _ = _plan(sampling)
        check(epi.ctx.lib.twosd_add_sampled_scenarios_vr(epi.ctx.h, epi.index, int(N), C.c_uint64(seed),
                                                          C.c_uint64(first_index), ptr(w), C.byref(plan)))
    epi.scenario_weight.extend([1.0] * N if w is None else list(w))


def get_scenarios(epi: sdEpigraph, first=0, count=None) -> np.ndarray:
    """Element values (template + stored delta) of scenarios [first, first+count)."""
    if count is None:
        count = epi.num_scenarios - first
    out = np.zeros((count, epi.ctx.k))
    check(epi.ctx.lib.twosd_get_scenarios(epi.ctx.h, epi.index, int(first), int(count), ptr(out)))
    return out


def solve_batch(epi: sdEpigraph, x, first=0, count=None, want_pi=True, want_y=False):
    """solve_problem! over scenarios [first, first+count) of epi at x -> (obj, y, pi, status)."""
    ctx = epi.ctx
    count = epi.num_scenarios - first if count is None else count
    obj = np.zeros(count)
    st = np.zeros(count, dtype=np.int32)
    pi = np.zeros((count, ctx.mv)) if want_pi else None
    y = np.zeros((count, ctx.n2)) if want_y else None
    check(ctx.lib.twosd_solve_batch(ctx.h, epi.index, ptr(_f64(x)), first, count, ptr(obj), ptr(pi), ptr(y), ptr(st)))
    return obj, y, pi, st


def solve_problem(ctx: SDContext, x, scenario):
    """solve_problem!(sp, x, scenario) -> (obj, y_opt, dual_opt) (smps_routines.jl:50-62).
    A non-optimal LP raises (the reference logs @error and returns junk duals)."""
    obj, y, pi, st = ctx.solve_values(x, ctx.scenario_values(scenario)[None, :], want_pi=True, want_y=True)
    return float(obj[0]), y[0], pi[0]


def evaluate(ctx: SDContext, first_stage_cost, x, values):
    """evaluate(sp1, sp2, sto, x; N) (smps_routines.jl:67-82) on given sampled values:
    c'x + (1/N) sum_w obj_w.  first_stage_cost: the stage-1 objective vector."""
    obj, _, _, _ = ctx.solve_values(x, values, want_pi=False)
    N = obj.shape[0]
    s2 = 0.0
    for o in obj:                      # s2_cost += 1/N*obj, in sample order (:79)
        s2 += 1.0 / N * o
    return float(np.dot(first_stage_cost, x)) + s2


def evaluate_sampled(ctx: SDContext, first_stage_cost, x, N, seed, first=0, count=None):
    """evaluate(sp1, sp2, sto, x; N) (smps_routines.jl:67-82) with the N scenarios drawn on
    the device (needs ctx.set_distributions): c'x + sum_w (1/N) obj_w in scenario order.
    first/count select a shard of the stream (the c'x term is added by every caller of
    a shard; multi-GPU: sqlp_amd.dist.evaluate_sharded)."""
    count = N - first if count is None else count
    s2 = C.c_double()
    check(ctx.lib.twosd_evaluate_sampled(ctx.h, ptr(_f64(x)), C.c_int64(N), C.c_int64(first), C.c_int64(count),
                                         C.c_uint64(seed), C.byref(s2)))
    return float(np.dot(first_stage_cost, x)) + s2.value


@dataclass(frozen=True)
class Moments:
    """struct twosd_moments: sample moments of the stage-2 objective over the n scenarios whose LP
    was optimal (n_bad: the others), reduced on the device in a fixed order and mergeable."""
    n: int = 0
    n_bad: int = 0
    mean: float = 0.0
    m2: float = 0.0
    min: float = float("inf")
    max: float = float("-inf")
    group: int = 1      # > 1: the observations are means of groups of `group` scenarios (Sampling)

    @property
    def n_scenarios(self) -> int:
        """Scenarios behind the n counted observations (n groups of `group`)."""
        return self.n * self.group

    @property
    def variance(self) -> float:
        """Sample variance (ddof = 1); nan for n < 2."""
        return self.m2 / (self.n - 1) if self.n >= 2 else float("nan")

    @property
    def std_error(self) -> float:
        """Standard error of the mean."""
        return float(np.sqrt(self.m2 / (self.n - 1) / self.n)) if self.n >= 2 else float("nan")

    def half_width(self, z: float = 1.959963984540054) -> float:
        """Half-width of the normal confidence interval of the mean (z: a normal quantile)."""
        return z * self.std_error

    def merge(self, other: "Moments") -> "Moments":
        """twosd_moments_merge(self, other): the moments of both samples together."""
        if self.group != other.group:
            raise ValueError(f"merge: moments over groups of {self.group} and of {other.group}")
        a, b, out = self._c(), other._c(), _lib.Moments()
        check(_lib.load().twosd_moments_merge(C.byref(a), C.byref(b), C.byref(out)))
        return Moments._of(out, self.group)

    def _c(self):
        return _lib.Moments(int(self.n), int(self.n_bad), float(self.mean), float(self.m2), float(self.min), float(self.max))

    @classmethod
    def _of(cls, m, group=1) -> "Moments":
        return cls(int(m.n), int(m.n_bad), float(m.mean), float(m.m2), float(m.min), float(m.max), int(group))


def _lp_status_ok(rc, raise_on_status):
    """check(rc), except that TWOSD_E_LP passes when the caller asked to see n_bad instead."""
    if rc != 0 and not (rc == -4 and not raise_on_status):
        check(rc)


def moments_of_values(ctx: SDContext, obj, status=None, group=1) -> Moments:
    """Moments of the caller's own objectives on the device (twosd_moments_of_values): entries
    whose status is not optimal are left out (n_bad) and never read into a sum.  group = G > 1
    (twosd_moments_of_values_grouped): the moments of the means of groups of G consecutive
    entries; a group counts when all of its entries are optimal, n and n_bad count groups."""
    obj = _f64(np.ravel(obj))
    st = None if status is None else np.ascontiguousarray(np.ravel(status), dtype=np.int32)
    if st is not None and st.shape != obj.shape:
        raise ValueError("status and obj differ in length")
    out = _lib.Moments()
    if int(group) == 1:
        check(ctx.lib.twosd_moments_of_values(ctx.h, C.c_int64(obj.size), ptr(obj), ptr(st), C.byref(out)))
    else:
        check(ctx.lib.twosd_moments_of_values_grouped(ctx.h, C.c_int64(obj.size), int(group), ptr(obj), ptr(st), C.byref(out)))
    return Moments._of(out, group)


def evaluate_moments(ctx: SDContext, first_stage_cost, x, seed, first, count, raise_on_status=True, sampling=None) -> Moments:
    """Moments of c'x + obj_w over scenarios [first, first+count) of the device-drawn stream `seed`
    (twosd_evaluate_moments: no objective leaves the device).  mean, min and max include c'x.
    raise_on_status=False returns the moments of the optimal scenarios when some LP is not
    optimal (their number is n_bad) instead of raising.  sampling: a Sampling plan
    (twosd_evaluate_moments_vr): the moments are then of the group means, n and n_bad in groups."""
    out = _lib.Moments()
    plan, G = _plan(sampling)
    if plan is None:
        rc = ctx.lib.twosd_evaluate_moments(ctx.h, ptr(_f64(x)), C.c_int64(first), C.c_int64(count), C.c_uint64(seed),
                                            C.byref(out))
    else:
        rc = ctx.lib.twosd_evaluate_moments_vr(ctx.h, ptr(_f64(x)), C.c_int64(first), C.c_int64(count), C.c_uint64(seed),
                                               C.byref(out), C.byref(plan))
    _lp_status_ok(rc, raise_on_status)
    return _shift(Moments._of(out, G), float(np.dot(first_stage_cost, x)))


def _shift(m: Moments, c: float) -> Moments:
    if m.n == 0 or c == 0.0:
        return m
    return Moments(m.n, m.n_bad, m.mean + c, m.m2, m.min + c, m.max + c, m.group)


def evaluate_paired(ctx: SDContext, first_stage_cost, xa, xb, seed, first, count, raise_on_status=True, sampling=None):
    """Two first-stage points on common random numbers (twosd_evaluate_paired): the same
    scenarios solved at xa and at xb -> (a, b, diff), diff the moments of the per-scenario
    difference of c'x + obj.  diff.half_width() is the error bar of "xa is better than xb".
    sampling: a Sampling plan (twosd_evaluate_paired_vr): all three over group means."""
    a, b, d = _lib.Moments(), _lib.Moments(), _lib.Moments()
    plan, G = _plan(sampling)
    if plan is None:
        rc = ctx.lib.twosd_evaluate_paired(ctx.h, ptr(_f64(xa)), ptr(_f64(xb)), C.c_int64(first), C.c_int64(count),
                                           C.c_uint64(seed), C.byref(a), C.byref(b), C.byref(d))
    else:
        rc = ctx.lib.twosd_evaluate_paired_vr(ctx.h, ptr(_f64(xa)), ptr(_f64(xb)), C.c_int64(first), C.c_int64(count),
                                              C.c_uint64(seed), C.byref(a), C.byref(b), C.byref(d), C.byref(plan))
    _lp_status_ok(rc, raise_on_status)
    ca, cb = float(np.dot(first_stage_cost, xa)), float(np.dot(first_stage_cost, xb))
    return _shift(Moments._of(a, G), ca), _shift(Moments._of(b, G), cb), _shift(Moments._of(d, G), ca - cb)


@dataclass(frozen=True)
class EvaluateCI:
    """Result of evaluate_ci: mean (c'x included) +- half_width over n observations: scenarios,
    or under a Sampling plan groups of `group` scenarios (n_bad likewise)."""
    mean: float
    half_width: float
    n: int
    n_bad: int
    converged: bool
    moments: Moments    # stage-2 part alone (without c'x)
    group: int = 1

    @property
    def n_scenarios(self) -> int:
        """Scenarios behind the n counted observations."""
        return self.n * self.group


def normal_quantile(confidence: float) -> float:
    """z of a two-sided normal interval (the library holds no inverse CDF)."""
    if not 0.0 < confidence < 1.0:
        raise ValueError("confidence must lie in (0, 1)")
    from statistics import NormalDist
    return NormalDist().inv_cdf(0.5 + 0.5 * confidence)


def evaluate_ci(ctx: SDContext, first_stage_cost, x, seed, batch=4096, n_max=1 << 20, confidence=0.95, rel_tol=1e-3,
                abs_tol=0.0, first=0, raise_on_status=True, z=None, sampling=None) -> EvaluateCI:
    """Sample the stream `seed` in batches until the confidence interval of c'x + E[obj] is tight
    (twosd_evaluate_ci): half-width <= max(abs_tol, rel_tol |mean|), or n_max scenarios.  z (a
    quantile of the caller's own, e.g. Student's t) overrides `confidence`.  sampling: a Sampling
    plan (twosd_evaluate_ci_vr): batch holds at least two whole groups, the rule runs on the
    moments of the group means and n counts groups (n_scenarios: scenarios)."""
    out = _lib.Moments()
    hw = C.c_double()
    conv = C.c_int()
    offset = float(np.dot(first_stage_cost, x))
    zq = normal_quantile(confidence) if z is None else float(z)
    plan, G = _plan(sampling)
    if plan is None:
        rc = ctx.lib.twosd_evaluate_ci(ctx.h, ptr(_f64(x)), C.c_uint64(seed), C.c_int64(first), C.c_int64(batch),
                                       C.c_int64(n_max), zq, float(rel_tol), float(abs_tol), offset,
                                       C.byref(out), C.byref(hw), C.byref(conv))
    else:
        rc = ctx.lib.twosd_evaluate_ci_vr(ctx.h, ptr(_f64(x)), C.c_uint64(seed), C.c_int64(first), C.c_int64(batch),
                                          C.c_int64(n_max), zq, float(rel_tol), float(abs_tol), offset,
                                          C.byref(out), C.byref(hw), C.byref(conv), C.byref(plan))
    _lp_status_ok(rc, raise_on_status)
    m = Moments._of(out, G)
    return EvaluateCI(offset + m.mean, hw.value, m.n, m.n_bad, bool(conv.value), m, G)


def evaluate_epigraph(cuts, incumbent_cut, x, total_scenario_weight, lower_bound, sense=MIN_SENSE):
    """Pointwise max (MIN sense) of the discounted cuts and the incumbent cut at x, floored by
    the lower bound; no epigraph weight (epigraph.jl:177-203)."""
    best = lower_bound
    x = np.asarray(x, dtype=np.float64)
    for cut in cuts:
        discount = cut.weight_mark / total_scenario_weight
        val = discount * (cut.alpha + float(np.dot(cut.beta, x))) + (1 - discount) * lower_bound
        if (sense == MIN_SENSE and val > best) or (sense != MIN_SENSE and val < best):
            best = val
    if incumbent_cut is not None:
        val = incumbent_cut.alpha + float(np.dot(incumbent_cut.beta, x))
        if (sense == MIN_SENSE and val > best) or (sense != MIN_SENSE and val < best):
            best = val
    return best


def evaluate_epigraph_weighted(epi: sdEpigraph, x, sense=MIN_SENSE):
    """objective_weight * evaluate_epigraph over the epigraph's cuts (epigraph.jl:205-219)."""
    return epi.objective_weight * evaluate_epigraph(epi.cuts, epi.incumbent_cut, x, epi.total_scenario_weight,
                                                    epi.lower_bound, sense=sense)


def evaluate_multi_epigraph(epis, x, sense=MIN_SENSE):
    """Sum of the weighted epigraph values (epigraph.jl:221-228)."""
    return sum(evaluate_epigraph_weighted(e, x, sense=sense) for e in epis)


INCUMBENT_SELECTION_Q = 0.2


@dataclass
class sdImprovementInfo:
    candidate_estimation: float
    incumbent_estimation: float
    required_improvement: float
    is_improved: bool


def check_improvement(f_last, f_current, f_cand, f_inc, x_candidate, x_incumbent, sense=MIN_SENSE):
    """Incumbent selection (improvement.jl:19-49).  f_cand / f_inc are the values of the
    common (first-stage) expression at the candidate / incumbent (evaluate_expr)."""
    ce = evaluate_multi_epigraph(f_current, x_candidate, sense) + f_cand
    ie = evaluate_multi_epigraph(f_current, x_incumbent, sense) + f_inc
    lce = evaluate_multi_epigraph(f_last, x_candidate, sense) + f_cand
    lie = evaluate_multi_epigraph(f_last, x_incumbent, sense) + f_inc
    req_impr = INCUMBENT_SELECTION_Q * (lce - lie)
    req = ie + req_impr
    improved = ce < req if sense == MIN_SENSE else ce > req
    return sdImprovementInfo(ce, ie, req_impr, improved)


def argmax_procedure(epi: sdEpigraph, x, dual_vertices: sdDualVertexSet, tie_rel=DEFAULT_TIE_REL):
    """(max_val, max_arg) over every scenario of epi (subprob.jl:141-169); max_arg holds
    0-based vertex indices into dual_vertices (the reference returns Refs to vectors)."""
    cut, mv, ma = _build_cut(epi, x, tie_rel, want_argmax=True)
    return mv, ma


def build_sasa_cut(epi: sdEpigraph, x, dual_vertices: sdDualVertexSet, tie_rel=DEFAULT_TIE_REL,
                   keep_picks=False) -> sdCut:
    """build_sasa_cut(epi, x, V) (epigraph.jl:125-146).  keep_picks: the cut carries a handle of
    its argmax picks (cut.picks, 4 bytes per scenario on the device) for reform_cuts; a cut of an
    epigraph without scenarios has none."""
    cut, _, _ = _build_cut(epi, x, tie_rel, want_argmax=False)
    if keep_picks and epi.num_scenarios > 0 and epi.total_scenario_weight > 0.0:
        cut.picks = keep_picks_of_last_cut(epi)
    return cut


# -- stored picks and bootstrap re-formation (the in-sample stopping rule's device part; the
#    reference's plugin/stopping_rule.jl is an empty file) ------------------------------------
def keep_picks_of_last_cut(epi: sdEpigraph) -> int:
    """twosd_picks_keep: a handle of the picks of the last cut built on epi."""
    h = C.c_int()
    check(epi.ctx.lib.twosd_picks_keep(epi.ctx.h, epi.index, C.byref(h)))
    epi._pick_handles.add(h.value)
    return h.value


def picks_info(ctx: SDContext, handle):
    """(epigraph index, scenarios, |V|) of a pick handle."""
    e, n, nv = C.c_int(), C.c_int(), C.c_int()
    check(ctx.lib.twosd_picks_info(ctx.h, int(handle), C.byref(e), C.byref(n), C.byref(nv)))
    return e.value, n.value, nv.value


def picks_get(ctx: SDContext, handle) -> np.ndarray:
    """The stored picks (0-based vertex indices) of a handle."""
    out = np.zeros(picks_info(ctx, handle)[1], dtype=np.int32)
    check(ctx.lib.twosd_picks_get(ctx.h, int(handle), ptr(out)))
    return out


def picks_release(ctx: SDContext, handle):
    check(ctx.lib.twosd_picks_release(ctx.h, int(handle)))


def picks_count(ctx: SDContext) -> int:
    """Live pick handles of the context."""
    n = C.c_int()
    check(ctx.lib.twosd_picks_count(ctx.h, C.byref(n)))
    return n.value


def bootstrap_count_of_word(u: int) -> int:
    """Poisson(1) count of a uniform 32-bit word (twosd_bootstrap_count_of_word; host code)."""
    return int(_lib.load().twosd_bootstrap_count_of_word(C.c_uint32(int(u))))


def bootstrap_counts(ctx: SDContext, M, seed, first_index, count, sampling=None) -> np.ndarray:
    """The device draw of the replicate counts of scenarios [first_index, first_index + count):
    uint8 (count, M).  sampling: a Sampling plan (twosd_bootstrap_counts_vr): whole groups are
    resampled, scenario g carries the count of group g // G; first_index and count are whole groups."""
    out = np.zeros((int(count), int(M)), dtype=np.uint8)
    if sampling is None:
        check(ctx.lib.twosd_bootstrap_counts(ctx.h, int(M), C.c_uint64(seed), C.c_uint64(first_index), C.c_int64(count),
                                             ptr(out)))
    else:
        plan, _ = _plan(sampling)
        check(ctx.lib.twosd_bootstrap_counts_vr(ctx.h, int(M), C.c_uint64(seed), C.c_uint64(first_index), C.c_int64(count),
                                                ptr(out), C.byref(plan)))
    return out


@dataclass
class ReformedCuts:
    """reform_cuts' result: row 0 the identity replicate, row 1 + b bootstrap replicate b."""
    alpha: np.ndarray          # (M + 1, H)
    beta: np.ndarray           # (M + 1, H, n1)
    weight_mark: np.ndarray    # (M + 1, H)
    total_weight: np.ndarray   # (M + 1,)

    def cut(self, b, j) -> sdCut:
        return sdCut(float(self.alpha[b, j]), self.beta[b, j], float(self.weight_mark[b, j]))


def _handles_of(cuts):
    hs = []
    for cut in cuts:
        h = cut.picks if isinstance(cut, (sdCut, sdTailCut)) else cut   # a pick handle or a tail handle, alike
        if h is None:
            raise ValueError("reform_cuts: a cut carries no picks (build it with keep_picks=True)")
        hs.append(int(h))
    return np.ascontiguousarray(hs, dtype=np.int32)


def reform_cuts(epi: sdEpigraph, cuts, M, seed, index_offset=0, sampling=None) -> ReformedCuts:
    """twosd_reform_cuts: every cut of `cuts` (sdCut with picks, or pick handles) re-formed from its
    picks under the identity weights (row 0) and M Poisson(1) bootstrap replicates of the scenario
    weights (seed; index_offset = the global index of the epigraph's first scenario).  sampling: the
    Sampling plan the epigraph was filled with (twosd_reform_cuts_vr): the replicates resample whole
    groups; index_offset, the epigraph's scenario count and every cut's are then whole groups."""
    ctx = epi.ctx
    hs = _handles_of(cuts)
    H, B = len(hs), int(M) + 1
    alpha = np.zeros((B, H))
    beta = np.zeros((B, H, ctx.n1))
    wm = np.zeros((B, H))
    tw = np.zeros(B)
    if sampling is None:
        check(ctx.lib.twosd_reform_cuts(ctx.h, epi.index, H, ptr(hs), int(M), C.c_uint64(seed), C.c_uint64(index_offset),
                                        ptr(alpha), ptr(beta), ptr(wm), ptr(tw)))
    else:
        plan, _ = _plan(sampling)
        check(ctx.lib.twosd_reform_cuts_vr(ctx.h, epi.index, H, ptr(hs), int(M), C.c_uint64(seed), C.c_uint64(index_offset),
                                           ptr(alpha), ptr(beta), ptr(wm), ptr(tw), C.byref(plan)))
    return ReformedCuts(alpha, beta, wm, tw)


def reform_last_ms(ctx: SDContext):
    """Device milliseconds of the last reform_cuts: [partial sums, finalize]."""
    out = np.zeros(2)
    check(ctx.lib.twosd_reform_last_ms(ctx.h, ptr(out)))
    return out


# -- risk measures: weighted quantiles, tail cuts, out-of-sample CVaR (risk.hip; the reference
#    optimises the expectation only) -----------------------------------------------------------
@dataclass(frozen=True)
class Quantile:
    """twosd_quantile_of_values' result: VaR and CVaR at `level`, and the integer weights
    tail_q = sum of q_s over value > var, total_q = Q; n_bad entries were left out."""
    var: float
    cvar: float
    tail_q: int
    total_q: int
    n_bad: int


def _level(level) -> float:
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError(f"level = {level} outside (0, 1)")
    return level


def quantile_of_values(ctx: SDContext, values, level, weights=None, status=None) -> Quantile:
    """VaR / CVaR at `level` of the caller's own values, selected on the device
    (twosd_quantile_of_values): integer weights q_s = rn(w_s 2^58 / sum w) (1 without weights),
    entries whose status is not optimal left out (n_bad), the threshold ceil(level Q) exact."""
    values = _f64(np.ravel(values))
    w = None if weights is None else _f64(np.ravel(weights))
    st = None if status is None else np.ascontiguousarray(np.ravel(status), dtype=np.int32)
    if (w is not None and w.shape != values.shape) or (st is not None and st.shape != values.shape):
        raise ValueError("weights / status and values differ in length")
    var, cvar = C.c_double(), C.c_double()
    tq, Q, nb = C.c_uint64(), C.c_uint64(), C.c_int64()
    check(ctx.lib.twosd_quantile_of_values(ctx.h, C.c_int64(values.size), ptr(values), ptr(w), ptr(st), float(level),
                                           C.byref(var), C.byref(cvar), C.byref(tq), C.byref(Q), C.byref(nb)))
    return Quantile(var.value, cvar.value, tq.value, Q.value, nb.value)


@dataclass(frozen=True)
class CutQuantile:
    """twosd_cut_quantile's result: VaR and CVaR of the last cut's scores under the scenario
    weights; tail_weight = the weight of the scenarios scoring above var."""
    var: float
    cvar: float
    tail_weight: float
    total_weight: float


def cut_quantile(epi: sdEpigraph, level) -> CutQuantile:
    """VaR / CVaR at `level` of the maximal scores of the last cut built on epi (what
    build_sasa_cut returns in max_val), under the scenario weights; no score leaves the device."""
    ctx = epi.ctx
    out = [C.c_double() for _ in range(4)]
    check(ctx.lib.twosd_cut_quantile(ctx.h, epi.index, _level(level), *[C.byref(o) for o in out]))
    return CutQuantile(*[o.value for o in out])


@dataclass
class sdTailCut:
    """cut_tail's result: tau >= d (alpha + beta'x - eta) with d = tail_weight / total_weight
    bounds the sample's E[(h - eta)+] from below; the zero cut with tail_weight 0 when no scenario
    scores above eta."""
    alpha: float
    beta: np.ndarray
    tail_weight: float
    total_weight: float
    eta: float
    picks: Optional[int] = None   # the tail handle (cut_tail(keep=True)), for reform_cuts

    @property
    def d(self) -> float:
        return self.tail_weight / self.total_weight


def cut_tail(epi: sdEpigraph, eta, keep=False) -> sdTailCut:
    """twosd_cut_tail: the last cut built on epi re-formed from its picks over the scenarios whose
    score exceeds eta (strictly), normalised by their weight.  keep: the result carries a tail
    handle of that set and its picks (keep_tail_of_last_cut)."""
    ctx = epi.ctx
    a, tw, W = C.c_double(), C.c_double(), C.c_double()
    beta = np.zeros(ctx.n1)
    check(ctx.lib.twosd_cut_tail(ctx.h, epi.index, float(eta), C.byref(a), ptr(beta), C.byref(tw), C.byref(W)))
    return sdTailCut(a.value, beta, tw.value, W.value, float(eta), keep_tail_of_last_cut(epi, eta) if keep else None)


def keep_tail_of_last_cut(epi: sdEpigraph, eta) -> int:
    """twosd_tail_keep: a handle of the tail of the last cut built on epi at eta -- the scenarios
    scoring above eta (cut_tail's set, bit for bit) in ascending order and their picks, compacted on
    the device (8 bytes per tail scenario).  reform_cuts takes it like a pick handle; it is released,
    counted and dropped like one."""
    h = C.c_int()
    check(epi.ctx.lib.twosd_tail_keep(epi.ctx.h, epi.index, float(eta), C.byref(h)))
    epi._pick_handles.add(h.value)
    return h.value


@dataclass(frozen=True)
class TailInfo:
    """twosd_tail_info's result: the cut's epigraph, scenarios and |V|, the tail's length and its eta."""
    epi: int
    n: int
    nv: int
    nt: int
    eta: float


def tail_info(ctx: SDContext, handle) -> TailInfo:
    e, n, nv, nt, eta = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_double()
    check(ctx.lib.twosd_tail_info(ctx.h, int(handle), C.byref(e), C.byref(n), C.byref(nv), C.byref(nt), C.byref(eta)))
    return TailInfo(e.value, n.value, nv.value, nt.value, eta.value)


def tail_get(ctx: SDContext, handle):
    """(scenario indices ascending, their picks) of a tail handle: two int32 arrays of length nt."""
    nt = tail_info(ctx, handle).nt
    scen, pick = np.zeros(nt, dtype=np.int32), np.zeros(nt, dtype=np.int32)
    check(ctx.lib.twosd_tail_get(ctx.h, int(handle), ptr(scen), ptr(pick)))
    return scen, pick


def tail_last_ms(ctx: SDContext) -> float:
    """Device milliseconds of the last keep_tail_of_last_cut."""
    ms = C.c_double()
    check(ctx.lib.twosd_tail_last_ms(ctx.h, C.byref(ms)))
    return ms.value


def risk_last_ms(ctx: SDContext):
    """Device milliseconds of [the last quantile selection, the last cut_tail]."""
    out = np.zeros(2)
    check(ctx.lib.twosd_risk_last_ms(ctx.h, ptr(out)))
    return out


@dataclass(frozen=True)
class EvaluateCVaR:
    """twosd_evaluate_cvar's result (c'x included in var and cvar): y holds the moments of
    Y = var + (obj - var)+ / (1 - level), whose mean is cvar."""
    var: float
    cvar: float
    n: int
    n_bad: int
    y: Moments

    @property
    def std_error(self) -> float:
        """Asymptotic standard error of cvar (the plain-sample one of Y)."""
        return self.y.std_error

    def half_width(self, z: float = 1.959963984540054) -> float:
        return z * self.std_error


def evaluate_cvar(ctx: SDContext, first_stage_cost, x, seed, first, count, level, raise_on_status=True,
                  sampling=None) -> EvaluateCVaR:
    """Out-of-sample VaR and CVaR at `level` of c'x + obj_w over scenarios [first, first+count) of
    the i.i.d. device stream `seed` (twosd_evaluate_cvar: no objective leaves the device).
    Variance-reduced plans are not supported: ValueError for a sampling= other than i.i.d."""
    if sampling is not None and (int(sampling.mode) != _lib.SAMPLING_IID or int(sampling.group) != 1):
        raise ValueError("evaluate_cvar: i.i.d. streams only (no variance-reduced plan)")
    out = _lib.Cvar()
    rc = ctx.lib.twosd_evaluate_cvar(ctx.h, ptr(_f64(x)), C.c_uint64(seed), C.c_int64(first), C.c_int64(count), _level(level),
                                     C.byref(out))
    _lp_status_ok(rc, raise_on_status)
    c = float(np.dot(first_stage_cost, x))
    return EvaluateCVaR(out.var + c, out.cvar + c, int(out.n), int(out.n_bad), _shift(Moments._of(out.y), c))


def reform_partial_len(ctx: SDContext, cuts, M):
    hs = _handles_of(cuts)
    a, b = C.c_int64(), C.c_int64()
    check(ctx.lib.twosd_reform_partial_len(ctx.h, len(hs), ptr(hs), int(M), C.byref(a), C.byref(b)))
    return a.value, b.value


def reform_partial(epi: sdEpigraph, cuts, M, seed, index_offset, total_weight, d_u64_ptr, d_f64_ptr, sampling=None):
    """This rank's part of reform_cuts into caller device buffers (reform_partial_len entries);
    total_weight: the global total scenario weight, the same on every rank.  sampling: as
    reform_cuts (twosd_reform_partial_vr); the rank then holds whole groups."""
    ctx = epi.ctx
    hs = _handles_of(cuts)
    if sampling is None:
        check(ctx.lib.twosd_reform_partial(ctx.h, epi.index, len(hs), ptr(hs), int(M), C.c_uint64(seed),
                                           C.c_uint64(index_offset), float(total_weight), C.c_void_p(d_u64_ptr),
                                           C.c_void_p(d_f64_ptr)))
    else:
        plan, _ = _plan(sampling)
        check(ctx.lib.twosd_reform_partial_vr(ctx.h, epi.index, len(hs), ptr(hs), int(M), C.c_uint64(seed),
                                              C.c_uint64(index_offset), float(total_weight), C.c_void_p(d_u64_ptr),
                                              C.c_void_p(d_f64_ptr), C.byref(plan)))


def reform_finalize(ctx: SDContext, cuts, M, total_weight, d_u64_ptr, d_f64_ptr) -> ReformedCuts:
    """The re-formed cuts from the ranks' summed partial buffers."""
    hs = _handles_of(cuts)
    H, B = len(hs), int(M) + 1
    alpha = np.zeros((B, H))
    beta = np.zeros((B, H, ctx.n1))
    wm = np.zeros((B, H))
    tw = np.zeros(B)
    check(ctx.lib.twosd_reform_finalize(ctx.h, H, ptr(hs), int(M), float(total_weight), C.c_void_p(d_u64_ptr),
                                        C.c_void_p(d_f64_ptr), ptr(alpha), ptr(beta), ptr(wm), ptr(tw)))
    return ReformedCuts(alpha, beta, wm, tw)


def release_unused_picks(epi: sdEpigraph, keep=()) -> int:
    """Release the pick handles of epi's context that belong to epi and are referenced neither by
    epi.cuts nor by epi.incumbent_cut (nor listed in `keep`); returns how many were released."""
    used = {int(h) for h in keep}
    for cut in list(epi.cuts) + [epi.incumbent_cut]:
        if cut is not None and cut.picks is not None:
            used.add(int(cut.picks))
    freed = 0
    for h in sorted(epi._pick_handles - used):
        picks_release(epi.ctx, h)
        epi._pick_handles.discard(h)
        freed += 1
    return freed


def _build_cut(epi, x, tie_rel, want_argmax):
    ctx = epi.ctx
    a = C.c_double()
    wm = C.c_double()
    beta = np.zeros(ctx.n1)
    N = epi.num_scenarios
    mv = np.zeros(N) if want_argmax else None
    ma = np.zeros(N, dtype=np.int32) if want_argmax else None
    check(ctx.lib.twosd_build_cut(ctx.h, epi.index, ptr(_f64(x)), float(tie_rel), C.byref(a), ptr(beta),
                                  C.byref(wm), ptr(mv), ptr(ma)))
    return sdCut(a.value, beta, wm.value), mv, ma


def solve_push(epi: sdEpigraph, x, first, count, want_obj=True):
    """Device-side solve_problem! + push! of the duals (no host round trip).  want_obj=False
    skips the copy of the objectives and statuses (sd_iteration! does not read them; a
    non-optimal scenario still raises); obj and st are then None."""
    ctx = epi.ctx
    obj = np.zeros(count) if want_obj else None
    st = np.zeros(count, dtype=np.int32) if want_obj else None
    ns = C.c_int()
    check(ctx.lib.twosd_solve_push(ctx.h, epi.index, ptr(_f64(x)), first, count, ptr(obj) if want_obj else None,
                                   ptr(st) if want_obj else None, C.byref(ns)))
    return obj, st, ns.value


@dataclass
class sdEpigraphInfo:
    """epigraph.jl:152-171: the cuts, incumbent cut and total weight of an epigraph at one
    moment (copies), for the incumbent test of the next step."""
    objective_weight: float
    cuts: list
    incumbent_cut: object
    total_scenario_weight: float
    lower_bound: float

    @classmethod
    def of(cls, epi: "sdEpigraph") -> "sdEpigraphInfo":
        return cls(epi.objective_weight, list(epi.cuts), epi.incumbent_cut, epi.total_scenario_weight,
                   epi.lower_bound)


def sd_iteration_solve(epis, scenario_values, x_candidate, x_incumbent, V: sdDualVertexSet, added_at=None):
    """algorithm.jl:45-55: for every epigraph i, add_scenario!(epi_i, w_i, 1.0), solve at
    x_candidate and at x_incumbent and push! both duals.  The duals are pushed in the
    reference's order (epi 1 cand, epi 1 inc, epi 2 cand, ...; for a block of several
    scenarios per epigraph: cand/inc per scenario in order).  scenario_values[i] is a
    (N_i x k) block of new scenarios for epigraph i.  added_at[i] (optional): the block was already
    added to epigraph i at that index (the feasibility rounds of master.sd_iteration run between
    the two).  Returns the vertex index of every pushed dual (the order above)."""
    pis = []
    for i, (epi, vals) in enumerate(zip(epis, scenario_values)):
        vals = np.atleast_2d(vals)
        if added_at is None:
            first = epi.num_scenarios
            add_scenarios(epi, vals, np.ones(vals.shape[0]))
        else:
            first = added_at[i]
        _, _, pc, _ = solve_batch(epi, x_candidate, first, vals.shape[0])
        _, _, pinc, _ = solve_batch(epi, x_incumbent, first, vals.shape[0])
        inter = np.empty((2 * vals.shape[0], pc.shape[1]))
        inter[0::2] = pc
        inter[1::2] = pinc
        pis.append(inter)
    return V.push_batch(np.vstack(pis))


def sd_iteration_cuts(epis, x_candidate, x_incumbent, V: sdDualVertexSet, update_incumbent_cut=True,
                      tie_rel=DEFAULT_TIE_REL, keep_picks=False):
    """algorithm.jl:79-85: build_sasa_cut at x_candidate appended to epi.cuts and, if
    update_incumbent_cut, at x_incumbent as epi.incumbent_cut.  keep_picks: every new cut carries
    its picks (build_sasa_cut)."""
    for epi in epis:
        epi.cuts.append(build_sasa_cut(epi, x_candidate, V, tie_rel, keep_picks=keep_picks))
        if update_incumbent_cut:
            epi.incumbent_cut = build_sasa_cut(epi, x_incumbent, V, tie_rel, keep_picks=keep_picks)


def sd_iteration_hot_path(epis, scenario_values, x_candidate, x_incumbent, V: sdDualVertexSet,
                          update_incumbent_cut=True, tie_rel=DEFAULT_TIE_REL):
    """The data-parallel part of sd_iteration! (algorithm.jl:45-55 and :79-85) in one call:
    sd_iteration_solve, the sdEpigraphInfo snapshot the reference takes between the two
    halves (algorithm.jl:76: after add_scenario!, before any new cut), sd_iteration_cuts.
    Returns the snapshot (epi_info_last) for check_improvement.  Cut removal by master
    multipliers (algorithm.jl:57-72) sits between the halves in the reference; callers with
    a master use the two halves directly (sqlp_amd.master.sd_iteration)."""
    sd_iteration_solve(epis, scenario_values, x_candidate, x_incumbent, V)
    info = [sdEpigraphInfo.of(e) for e in epis]
    sd_iteration_cuts(epis, x_candidate, x_incumbent, V, update_incumbent_cut, tie_rel)
    return info
