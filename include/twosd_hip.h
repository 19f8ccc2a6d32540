/*
 * twosd_hip.h -- C ABI of libtwosd_hip.so, the MI355X (gfx950) implementation of the
 * TwoSD per-iteration scenario-subproblem + cut-generation hot path.
 *
 * Reference: yhz0/SQLP (module TwoSD, pure Julia) @ 2025-02-19.  The reference has no
 * FFI/plugin API for this path (src/sd_algorithm/plugin/ holds 0-byte files); the
 * entry points below are what a Julia `ccall` shim binds to add
 * accelerated methods for the same generic functions.  Each entry cites the reference
 * function it replaces.
 *
 * Conventions
 *   - All calls are synchronous: outputs are valid on return.  Host buffers are owned by
 *     the caller; the library copies in and out.  Device memory is owned by the context.
 *   - Return value: TWOSD_OK (0) or a negative TWOSD_E_* code; twosd_last_error() gives a
 *     thread-local message.  A context is not re-entrant; distinct contexts are
 *     independent (one context per GPU / process).
 *   - Indices: `index_base` = 1 accepts Julia's 1-based SparseMatrixCSC arrays directly.
 *   - Stage-2 LP of one scenario w at first-stage x (smps_routines.jl:50-62):
 *         min q'y  s.t.  W y  (G: >=, L: <=, E: ==)  r_w - T_w x,   y >= 0
 *     duals pi follow JuMP's MIN convention (G rows >= 0, L rows <= 0, E free;
 *     pi = d obj / d rhs), so obj = pi . (r_w - T_w x).
 *   - Variables of the simplex basis ("head"): j < n2 is structural y_j; j = n2 + i is the
 *     slack of row i.
 *   - General bounds lo <= y <= hi (twosd_set_template): the library solves the canonical LP of
 *     twosd_canonical_form (y' >= 0, m_lp = m2 + nb rows, n_lp columns; nb = boxed variables),
 *     see twosd_lp_shape.  Callers see:
 *       y            in their own space (n2 entries, every one within its bounds);
 *       objectives   of their own LP (obj[], twosd_last_objective, twosd_evaluate_sampled,
 *                    max_val[], alpha all include the shift's constant c0 = q.s);
 *       dual vectors of length mv = m_lp = m2 + nb: the m2 row duals (JuMP's convention), then
 *                    one multiplier <= 0 per boxed variable (ascending j), with
 *                        obj = v . [ r_w - T_w x - W s ; hi - lo ] + c0
 *                    (s = the shift point of each column: lo, hi of a (-inf, hi] column, or 0).
 *                    pi of twosd_solve_batch / twosd_solve_values and the vectors of
 *                    twosd_dvs_push / twosd_dvs_get have that length;
 *       basis heads  (set_basis, get_basis, pool_*) in the LP's numbering: m_lp entries, j < n_lp
 *                    an LP column, j = n_lp + i the slack of LP row i;
 *       scenario values in their own space (the caller's r, never the shifted one).
 *     With every bound [0, +inf) all of this equals m2 / n2 and the template is the caller's own.
 */
#ifndef TWOSD_HIP_H
#define TWOSD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct twosd_ctx twosd_ctx;

enum {
    TWOSD_OK = 0,
    TWOSD_E_ARG = -1,        /* bad argument (sizes, indices, NULL)          */
    TWOSD_E_DEVICE = -2,     /* HIP runtime / kernel launch failure           */
    TWOSD_E_STATE = -3,      /* call out of order (e.g. no template yet)      */
    TWOSD_E_LP = -4,         /* LP not solved to optimality (see status[])    */
    TWOSD_E_UNSUPPORTED = -5 /* template outside the kernel's envelope        */
};

/* per-scenario LP status (status[] outputs) */
enum { TWOSD_LP_OPTIMAL = 0, TWOSD_LP_INFEASIBLE = 1, TWOSD_LP_ITER_LIMIT = 2, TWOSD_LP_NUMERIC = 3 };

/* Thread-local message for the last failing call on this thread. */
const char *twosd_last_error(void);

/* Library version string. */
const char *twosd_version(void);

/* Create a context on HIP device `device` (one context per GPU / rank). */
int twosd_create(int device, twosd_ctx **out);
int twosd_destroy(twosd_ctx *ctx);

/*
 * Stage-2 template (replaces extract_coefficients, subprob.jl:15-69, and the JuMP model
 * held by spStageProblem, prob.jl:10-15).
 *   T: m2 x n1 CSC (colptr[n1+1], rowval[nnzT], nzval[nnzT]); W: m2 x n2 CSC.
 *   q[n2], r[m2], sense[m2] in {'G','L','E'}, ylb/yub[n2] (NULL: 0 / +inf; -inf / +inf for an
 *   absent bound).  Bounds other than [0, +inf) are removed by twosd_canonical_form and every
 *   kernel runs on the canonical LP (the reference only warns on them and drops the bound
 *   multipliers from its cuts, subprob.jl:19-26; here a dual vertex carries them, see the
 *   conventions above).  A template whose bounds are all [0, +inf) is used as given.  The
 *   kernel envelope (1024 rows, the column slots, the LDS slice) applies to the LP's sizes:
 *   each boxed variable costs one row.  TWOSD_E_ARG for bounds that are no interval (lo > hi,
 *   NaN, lo = +inf, hi = -inf).
 * Re-setting the template clears basis, scenarios, dual vertex set and cuts, and releases every
 * device array sized for the old template.  Statistics and heuristics start as on a fresh
 * context: the twosd_last_* getters, timings and refresh times read zero or their defaults, and
 * the push-mode choice and the automatic training pivot cap keep nothing of the old template.
 * Caller settings (twosd_set_refresh_kcap, TWOSD_KMAX) stay.
 */
int twosd_set_template(twosd_ctx *ctx, int m2, int n1, int n2,
                       const int64_t *T_colptr, const int64_t *T_rowval, const double *T_nzval,
                       const int64_t *W_colptr, const int64_t *W_rowval, const double *W_nzval,
                       const double *q, const double *r, const char *sense,
                       const double *ylb, const double *yub, int index_base);

/* Sizes of the LP the kernels solve for the current template: rows m_lp = m2 + n_bound_rows,
 * columns n_lp, bound rows (= boxed variables).  (m2, n2, 0) when every bound is [0, +inf).
 * Dual vectors and basis heads have m_lp entries.  Outputs nullable. */
int twosd_lp_shape(twosd_ctx *ctx, int *m_lp, int *n_lp, int *n_bound_rows);

/*
 * Canonical form of a stage-2 LP with general bounds (host code only: no context, no GPU call;
 * twosd_set_template applies it).  Per column j with lo = ylb[j], hi = yub[j]:
 *   [0, +inf)   unchanged                   [lo, +inf)   y = lo + y'
 *   (-inf, hi]  y = hi - y' (column and cost negated)
 *   free        y = y+ - y-, the y- columns appended after the kept columns, ascending j
 *   lo = hi     the column leaves the LP, y_j = lo
 *   [lo, hi]    y = lo + y' and one 'L' row y' <= hi - lo, appended after the m2 rows, ascending j
 * With s the shift point (lo; hi of the negated kind; else 0): out_r = [r - W s ; hi - lo] (the
 * columns with s != 0 in ascending j, entries in CSC order), *c0 = q.s, and T gains zero rows.
 * Outputs (caller-allocated for the worst case; each nullable): out_colptr[2 n2 + 1],
 * out_rowval / out_nzval[2 nnz(W) + n2], out_q[2 n2], out_r / out_sense[m2 + n2] -- *n_lp + 1,
 * nnz, *n_lp and *m_lp entries are written, indices in index_base.  The column table maps a
 * solution back: y_j = col_off[j] + col_sign[j] * y'[col_src[j]] - y'[col_src2[j]], an index of -1
 * (either base) meaning the term is absent; box_col[b] is the column of bound row m2 + b.  With
 * every bound [0, +inf) the outputs equal the inputs bit for bit and *n_bound_rows = 0.
 */
int twosd_canonical_form(int m2, int n2, const int64_t *W_colptr, const int64_t *W_rowval, const double *W_nzval,
                         const double *q, const double *r, const char *sense, const double *ylb, const double *yub,
                         int index_base, int *m_lp, int *n_lp, int *n_bound_rows, int64_t *out_colptr,
                         int64_t *out_rowval, double *out_nzval, double *out_q, double *out_r, char *out_sense,
                         double *c0, int *col_src, double *col_sign, double *col_off, int *col_src2, int *box_col);

/*
 * Random element positions of a scenario (spSmpsScenario entries, smps_sto.jl:135):
 * element e sits at stage-2 row row[e] (a row of the caller's template: < m2, never a bound
 * row); col[e] = -1 for an RHS entry, else the first-stage column of a T entry
 * (delta_coefficients, subprob.jl:104-121).  The listing fixes the columns of the value arrays
 * only: every decision uses the canonical element order (ascending row, RHS first, then T columns
 * ascending).  An element listed twice is refused with TWOSD_E_ARG (the reference keeps the last
 * write, subprob.jl:114-117); a refused call leaves k and the positions as they were.
 */
int twosd_set_random_positions(twosd_ctx *ctx, int k, const int *row, const int *col, int index_base);

/*
 * Warm-start basis shared by every scenario (dual feasible for all RHS).
 * twosd_compute_basis solves the LP at x for the scenario `values` (k entries; NULL =
 * template rhs) from the slack basis once on the host and installs its optimal basis.
 * twosd_set_basis installs a caller-provided basis (m2 variable indices, 0-based).
 */
int twosd_compute_basis(twosd_ctx *ctx, const double *x, const double *values);
int twosd_set_basis(twosd_ctx *ctx, const int *head);
int twosd_get_basis(twosd_ctx *ctx, int *head);

/* Warm-start basis pool (no reference counterpart: the reference warm-starts each
 * solve from the solver's previous basis, smps_routines.jl:50-62).  With only the
 * RHS random, every optimal basis of one scenario is dual feasible for all of them;
 * the LP kernel starts each scenario from the pool basis with the least primal
 * infeasibility.  Results are the same optimal vertices (same tie rules) -- only
 * the pivot count changes.  set_basis / compute_basis reset the pool to one basis.
 *   pool_add_basis: append a (dual-feasible) basis; *added = 0 if already present.
 *   pool_build: solve training scenarios [first, first+count) of epigraph epi at x
 *     and add their optimal bases, most frequent first, up to max_pool bases. */
int twosd_pool_add_basis(twosd_ctx *ctx, const int *head, int *added);
int twosd_pool_build(twosd_ctx *ctx, int epi, const double *x, int first, int count, int max_pool,
                     int *pool_size);
/* Two-level pool selection: level 1 over pool[0, level1), level 2 over the ncand bases
 * that a flat selection over the whole pool picks most often for the training scenarios
 * [first, first+count) of epi at x sharing the level-1 pick.  Cuts the selection cost of a
 * large pool to about that of its first level1 bases.  level1 = 0: flat selection;
 * ncand <= 1024.  Reset by any change of the pool.  The lists themselves are counted on the
 * host by the next two-level selection while its level-1 pass runs (twosd_pool_set_candidates
 * likewise): an allocation failure of their upload is reported by that solve. */
int twosd_pool_build_candidates(twosd_ctx *ctx, int epi, const double *x, int first, int count, int level1,
                                int ncand);
/* Rebuild the pool at x: solve the training scenarios [first, first+count) of epi at x from
 * the current pool and replace the pool by the primary basis plus their max_pool - 1 most
 * frequent optimal bases (ties: first occurrence).  A pool's bases are optimal near the x they
 * were harvested at, so a first-stage point far from the last one (an SD candidate, the x
 * of an evaluate) gets a pool of its own.  B^{-1} of each new basis is composed from its start
 * basis and the eta file of its training solve (no refactorisation), on the device by default
 * (TWOSD_REFRESH_HOST=1: on the host, then uploaded; same pool).  Selection becomes flat
 * (candidate lists reset).  last_refresh_ms: [training solves, basis keys + selection, pool
 * build (device; host path: composition), host upload (host path only), total] of the last
 * refresh. */
int twosd_pool_refresh(twosd_ctx *ctx, int epi, const double *x, int first, int count, int max_pool,
                       int *pool_size);
int twosd_last_refresh_ms(twosd_ctx *ctx, double *ms5);

/* Distributed refresh (one rank per GPU, the pool replicated; no reference counterpart: the
 * reference is single-process).  The twosd_pool_refresh of all ranks' training scenarios, split:
 *   1. twosd_refresh_train: solve this rank's training slice [first, first+count) of epi at x;
 *      *n_bases = its distinct optimal bases; box_lo/box_hi[k] (nullable) = the slice's delta box.
 *      twosd_refresh_train_bases: their 64-bit keys, counts and first scenarios (ascending).
 *   2. the caller all-gathers (keys, counts, first scenarios) and selects, identically on every
 *      rank, the max_pool - 1 most frequent bases (ties: first occurrence in rank order), each
 *      owned by the rank of its first occurrence.
 *   3. twosd_refresh_build_local: compose B^{-1} of the n_own bases this rank owns (its first
 *      scenarios reps[], in selection order) into a pack of *pack_bytes bytes;
 *      twosd_refresh_pack copies it to a caller DEVICE buffer for the all-gather.
 *   4. twosd_refresh_assemble: from the G gathered packs (DEVICE, `stride` bytes apart, rank
 *      order), the pool = primary + the sources order[0, R) (source ids: 1 + the rank-major
 *      position of a base among all packs), with the union box_lo/box_hi[k] of the slices.
 *      R = 0 (no optimal training scenario on any rank) keeps the current pool, as
 *      twosd_pool_refresh does.
 * Selection becomes flat; twosd_pool_candidate_picks / twosd_pool_set_candidates split the
 * two-level candidate lists the same way (picks of each rank's slice, lists from all picks). */
int twosd_refresh_train(twosd_ctx *ctx, int epi, const double *x, int first, int count, int *n_bases, double *box_lo,
                        double *box_hi);
/* The training solve of step 1 under a cap the ranks agree on: kcap > 0 pivots (<= 0: none), one
 * launch, no retry; *n_optimal = training scenarios of the slice that ended optimal.  The caller
 * derives kcap from every rank's twosd_refresh_cap_stats (pivot sum and size of the last batch of
 * >= 4096 scenarios: 3 x the global mean, at least 32) and, when fewer than half of ALL ranks'
 * training scenarios ended optimal, calls it again with kcap = 0 on every rank -- the rule
 * twosd_pool_refresh applies to one rank, decided once for all of them. */
int twosd_refresh_train_ex(twosd_ctx *ctx, int epi, const double *x, int first, int count, int kcap, int *n_bases,
                           int *n_optimal, double *box_lo, double *box_hi);
int twosd_refresh_cap_stats(twosd_ctx *ctx, int64_t *pivots_sum, int64_t *scenarios);
/* The training pivot cap twosd_pool_refresh would use for a last large batch of `scenarios`
 * solves with `pivots_sum` pivots in all, under this context's setting (and TWOSD_TRAIN_KCAP):
 * > 0 the setting, < 0 none (0), auto max(32, ceil(3 sum / n)).  The distributed refresh calls it
 * with the all-reduced sums, so every rank and the single-rank refresh apply one rule.  Host code
 * only; ctx may be NULL (setting 0). */
int twosd_training_cap(twosd_ctx *ctx, int64_t pivots_sum, int64_t scenarios, int *cap);
/* Step 2 of the distributed refresh, identical on every rank (host code, no context): over the n
 * bases all ranks list (twosd_refresh_train_bases, concatenated in rank order; rank_of[i] = the
 * listing rank), a key listed by several ranks counts the sum of its counts and belongs to its
 * first occurrence; the min(distinct, max_pool - 1) largest totals, ties by first occurrence, go
 * to owner[] / rep[] (the owning rank and its first scenario), *npick of them. */
int twosd_select_refresh_bases(const uint64_t *keys, const int64_t *counts, const int64_t *reps, const int32_t *rank_of,
                               int n, int max_pool, int64_t *owner, int64_t *rep, int *npick);
int twosd_refresh_train_bases(twosd_ctx *ctx, uint64_t *keys, int *counts, int *reps);
int twosd_refresh_build_local(twosd_ctx *ctx, int n_own, const int *reps, int64_t *pack_bytes);
int twosd_refresh_pack(twosd_ctx *ctx, void *d_dst);
int twosd_refresh_assemble(twosd_ctx *ctx, int G, const void *d_packs, int64_t stride, int R, const int *order,
                           const double *box_lo, const double *box_hi, int *pool_size);
int twosd_pool_candidate_picks(twosd_ctx *ctx, int epi, const double *x, int first, int count, int level1, int *p1,
                               int *pf);
int twosd_pool_set_candidates(twosd_ctx *ctx, int level1, int ncand, int n, const int *p1, const int *pf);
int twosd_pool_size(twosd_ctx *ctx, int *size);
int twosd_pool_get(twosd_ctx *ctx, int p, int *head);
/* Pool basis each scenario of the last LP batch started from (first N of it; 0 = the
 * primary basis, also after a pool start was retried from it). */
int twosd_last_pool_picks(twosd_ctx *ctx, int N, int *picks);

/* Drop the per-x data cached from the last x (x_B of every pool basis, coef_e(x), the
 * pool-selection stream, the cut's per-x products); the next call at any x rebuilds it.
 * Results never depend on it -- benchmarks call it so each pass pays its per-x setup. */
int twosd_invalidate_x(twosd_ctx *ctx);

/* Epigraphs (sdEpigraph, epigraph.jl:17-61): per-epigraph scenario pool + weights. */
int twosd_epigraph_create(twosd_ctx *ctx, int *epi_out);
/* add_scenario!(epi, w, weight) batched (epigraph.jl:81-96): values[N*k] are the
 * scenario's element values in position order; weights[N] (NULL = all 1.0). */
int twosd_add_scenarios(twosd_ctx *ctx, int epi, int N, const double *values, const double *weights);
int twosd_epigraph_info(twosd_ctx *ctx, int epi, int *num_scenarios, double *total_weight);

/*
 * On-device scenario sampling (rand(rng, sto), smps_sto.jl:117-149).
 * set_distributions: one distribution per random element (position order): kind[e] =
 *   0 DISCRETE (nsupport[e] (value, probability) pairs, concatenated over elements in
 *   values/probs; sorted by value like DiscreteNonParametric), 1 NORMAL (param0 = mean,
 *   param1 = VARIANCE: Normal(mean, sqrt(variance)), smps_sto.jl:122-125), 2 UNIFORM
 *   (param0 = left, param1 = right).  Reset by twosd_set_random_positions.
 * add_sampled_scenarios: appends N i.i.d. scenarios to epigraph epi (weights NULL = 1.0).
 *   Element e of scenario number first_index + s is drawn from Philox4x32-10(counter =
 *   (index, e), key = seed), so a stream is reproducible under any sharding.
 * get_scenarios: element values (template + stored delta) of scenarios [first, first+count).
 */
int twosd_set_distributions(twosd_ctx *ctx, int k, const int *kind, const int *nsupport, const double *values,
                            const double *probs, const double *param0, const double *param1);
int twosd_add_sampled_scenarios(twosd_ctx *ctx, int epi, int N, uint64_t seed, uint64_t first_index,
                                const double *weights);
int twosd_get_scenarios(twosd_ctx *ctx, int epi, int first, int count, double *values);

/*
 * Joint discrete distributions (SMPS BLOCKS DISCRETE / SCENARIOS DISCRETE).
 * A block is an ordered list of member elements e_0, e_1, ..., e_{n-1}: indices into the
 * random-position layout in the order the caller lists them, not necessarily contiguous or
 * ascending.  It has R >= 1 realisations in the caller's order; realisation r has probability
 * p_r >= 0 and one value per member, V[r][j].  Realisations are not sorted, not deduplicated and
 * not normalised (as DISCRETE treats its probabilities).  The block's lead is e_0.
 *
 * For global scenario index g all members use the words of Philox counter (g_lo, g_hi, lead, 0)
 * under key seed; the element word of an element outside a block is its own index, so no two draw
 * units share a counter.  With u1 = u01(w0, w1), the realisation index is the DISCRETE walk over
 * the block's probabilities,
 *     i = 0, cp = p_0; while (cp <= u && i < R - 1) cp = cp + p_{++i}      (plain fp64 additions)
 * and member e_j stores V[i][j] - template_value(e_j).  Under a sampling plan (below):
 *   IID         u = u1.
 *   ANTITHETIC  both members of pair g >> 1 use the words of index 2 (g >> 1); the odd member walks
 *               at 1 - u1.
 *   LHS         the permutation is that of (LHS block b, lead), u1 that of (g, lead), and
 *               u = min((perm[j] + u1) / S, 1 - 2^-53): the LHS formula with lead in place of e.
 * The library finds i by binary search in the walk's running sums (built with the same sequential
 * additions): the first i whose sum exceeds u, else R - 1.  The sums never decrease, so this is
 * the walk's index exactly, also where u equals a sum, across zero-probability realisations and
 * with total mass below 1.
 * Consequences: a one-member block whose values ascend is, bit for bit, the DISCRETE stream of
 * that element under all three plans; and a stream stays a pure function of (seed, global index,
 * element, plan, tables), so any sharding on group boundaries reproduces it.
 *
 * set_distributions_joint: kind / nsupport / values / probs / param0 / param1 as in
 *   twosd_set_distributions, where kind[e] = TWOSD_DIST_BLOCK marks a block member (nsupport[e] is
 *   ignored, it owns no entries of values / probs).  Block b has members
 *   members[member_off[b] .. member_off[b + 1]), nreal[b] realisations, its probabilities
 *   concatenated in block_probs and its values, realisation-major [nreal][n_members], in
 *   block_values.  nblocks == 0 is twosd_set_distributions; that call itself still refuses kind 3,
 *   and a later call of it drops the blocks.  Reset like the other tables (twosd_set_template,
 *   twosd_set_random_positions).
 *   TWOSD_E_ARG, leaving the previous tables in use, for: an element of kind 3 that is in no
 *   block; an element in two blocks or twice in one; a member whose kind is not 3; nreal < 1; an
 *   empty block; a negative or non-finite probability; a non-finite value; a member index outside
 *   [0, k).  TWOSD_E_UNSUPPORTED when the probabilities or the values of all blocks together
 *   exceed 2^31 - 1 entries (table offsets are 32-bit).
 */
#define TWOSD_DIST_BLOCK 3
int twosd_set_distributions_joint(twosd_ctx *ctx, int k, const int *kind, const int *nsupport, const double *values,
                                  const double *probs, const double *param0, const double *param1, int nblocks,
                                  const int *member_off, const int *members, const int *nreal, const double *block_probs,
                                  const double *block_values);

/*
 * Correlated continuous elements (SMPS BLOCKS LINTR).  Every member of a LINTR
 * block is an affine function of a few independent latent variables, v = c + H xi:
 *   - n >= 1 member elements e_0 .. e_{n-1}: indices into the random-position layout in the
 *     caller's order, not necessarily contiguous or ascending; one constant c_j per member;
 *   - q >= 1 latent variables, each DISCRETE, NORMAL(mean, variance) or UNIFORM(left, right) with
 *     the parameters and the validation of twosd_set_distributions;
 *   - a sparse n x q matrix H in CSR, latent indices ascending within a row, entries kept as
 *     given (explicit zeros included).
 * Latent words.  The latents of all LINTR blocks are numbered 0 .. Q-1 in block order, and latent
 * l draws as if it were element k + l of an independent layout of k + Q elements: scenario words
 * from Philox counter (g_lo, g_hi, k + l, 0), LHS permutation words from (b_lo, b_hi, k + l,
 * 2 + (i >> 2)), and the plan's inversion of an element (Box-Muller under IID and ANTITHETIC with
 * z negated for the odd member, the inverse normal CDF under LHS, the DISCRETE walk, the
 * two-rounding UNIFORM).  Its values are bit for bit those of columns k .. k+Q-1 of such a
 * layout.  Elements and block leads are below k, so no latent shares a counter with them.
 * Member value.  v = c_j; for each CSR entry (l, h) of row j, in order: v = v + (h * xi_l), every
 * product and every sum rounded to nearest, no fused multiply-add.  Stored delta = v -
 * template_value(e_j).
 * A stream stays a pure function of (seed, global index, element, plan, tables): any sharding on
 * group boundaries reproduces it, and the library's internal chunking of the latent pass (a
 * scratch of at most 64 MiB; TWOSD_LINTR_CHUNK = scenarios per chunk is a test hook) is invisible.
 * INDEP elements, discrete blocks (kind 3) and LINTR blocks coexist in one layout; a context
 * without LINTR blocks launches what it launched before them, with the same bits.
 *
 * set_distributions_lintr: the arguments of twosd_set_distributions_joint, where kind[e] =
 *   TWOSD_DIST_LINTR marks a LINTR member (it owns no entries of values / probs), plus the LINTR
 *   blocks.  lintr == NULL or lintr->nblocks == 0 is twosd_set_distributions_joint.  Block b has
 *   members members[member_off[b] .. member_off[b + 1]) with constants[] alongside, and latents
 *   latent_off[b] .. latent_off[b + 1]) of the global numbering; latent_kind / latent_nsupport /
 *   latent_param0 / latent_param1 have one entry per latent and latent_values / latent_probs the
 *   concatenated supports of the DISCRETE ones, all as twosd_set_distributions reads an element.
 *   row_ptr (one entry per member of all blocks, plus one) / col / val are one CSR over the member
 *   rows in members[] order; col is the latent's index within its block, in [0, q).
 *   Reset like the other tables; twosd_set_distributions and twosd_set_distributions_joint drop
 *   the LINTR tables.  TWOSD_E_ARG, naming the block, element or latent and leaving the previous
 *   tables in use, for: an element of kind 4 that is in no LINTR block; a member in two blocks or
 *   twice in one; a member whose kind is not 4; a member index outside [0, k); an empty block;
 *   q < 1; a column outside [0, q) or columns not strictly ascending within a row; a non-finite
 *   constant or coefficient; latent parameters twosd_set_distributions would refuse.
 *   TWOSD_E_UNSUPPORTED for k + Q >= 2^31 or latent supports past 2^31 - 1 entries.
 *   The selection key's spread of a member is sqrt(2 / pi) sqrt(sum_l h^2 Var xi_l): a scale (the
 *   mean absolute deviation of a normal variable of that variance), not a bound.
 */
#define TWOSD_DIST_LINTR 4
typedef struct twosd_lintr {
    int nblocks;
    const int *member_off;        /* nblocks + 1 */
    const int *members;           /* M = member_off[nblocks] */
    const double *constants;      /* M */
    const int *latent_off;        /* nblocks + 1 */
    const int *latent_kind;       /* Q = latent_off[nblocks] */
    const int *latent_nsupport;   /* Q */
    const double *latent_values;  /* sum of nsupport over the DISCRETE latents */
    const double *latent_probs;
    const double *latent_param0;  /* Q */
    const double *latent_param1;  /* Q */
    const int *row_ptr;           /* M + 1 */
    const int *col;               /* row_ptr[M] */
    const double *val;            /* row_ptr[M] */
} twosd_lintr;
int twosd_set_distributions_lintr(twosd_ctx *ctx, int k, const int *kind, const int *nsupport, const double *values,
                                  const double *probs, const double *param0, const double *param1, int nblocks,
                                  const int *member_off, const int *members, const int *nreal, const double *block_probs,
                                  const double *block_values, const twosd_lintr *lintr);

/*
 * Variance-reduced scenario streams (no reference counterpart: the reference's readme lists
 * "Implement SMPS sampling methods (antithetic, stratified)" as open).  A sampling plan makes
 * groups of `group` = G consecutive global scenario indices [G b, G b + G) dependent; a stream
 * stays a pure function of (seed, global index, element, plan), so any sharding on group
 * boundaries reproduces it.  With u1, u2 the uniforms the i.i.d. sampler forms for (index g,
 * element e) from Philox counter (g_lo, g_hi, e, 0):
 *   IID         the stream of twosd_add_sampled_scenarios, bit for bit (a NULL plan means IID).
 *   ANTITHETIC  pair p = g >> 1; both members use the words of index 2p.  The even member is the
 *               i.i.d. draw of index 2p; the odd member mirrors it: DISCRETE and UNIFORM at
 *               1 - u1, NORMAL with the Box-Muller z negated.
 *   LHS         block b = g / S, position j = g % S: per (b, e) a uniform random permutation perm of
 *               0..S-1 (inside-out Fisher-Yates: for i = 1..S-1, t = mulhi32(word_i, i + 1),
 *               perm[i] = perm[t], perm[t] = i; word_i = word i & 3 of Philox counter
 *               (b_lo, b_hi, e, 2 + (i >> 2))), and member j draws at
 *               u = min((perm[j] + u1(g, e)) / S, 1 - 2^-53): DISCRETE and UNIFORM as the i.i.d.
 *               sampler at u, NORMAL mean + sd * Phi^-1(max(u, 2^-54)).
 * Every call that takes a plan requires its first index, its count and its batch to be multiples
 * of G; TWOSD_E_ARG otherwise, and for an unknown mode, a group that contradicts the mode
 * (IID: 1, ANTITHETIC: 2) or S outside [2, 256].
 */
#define TWOSD_SAMPLING_IID        0   /* group 1 */
#define TWOSD_SAMPLING_ANTITHETIC 1   /* group 2 */
#define TWOSD_SAMPLING_LHS        2   /* group S, 2 <= S <= 256, any integer */
typedef struct twosd_sampling { int mode; int group; } twosd_sampling;

/* twosd_add_sampled_scenarios under a sampling plan (NULL / IID: that call itself). */
int twosd_add_sampled_scenarios_vr(twosd_ctx *ctx, int epi, int N, uint64_t seed, uint64_t first_index,
                                   const double *weights, const twosd_sampling *plan);

/* evaluate(sp1, sp2, sto, x; N) (smps_routines.jl:67-82), stage-2 part, on device-drawn
 * scenarios [first, first+count) of the stream `seed` (a shard of N_total):
 * *s2 = sum in index order of (1/N_total) * obj.  The caller adds c'x (and, across ranks,
 * the shards' s2 in rank order).  TWOSD_E_LP if any LP is not optimal. */
int twosd_evaluate_sampled(twosd_ctx *ctx, const double *x, int64_t N_total, int64_t first, int64_t count,
                           uint64_t seed, double *s2);

/*
 * Out-of-sample recourse cost with its error bar (no reference counterpart: evaluate,
 * smps_routines.jl:67-82, returns the mean alone; ssn_test.jl:50-57 sets it against the cuts'
 * lower bound).  Sample moments of the stage-2 objective over scenarios of a stream, reduced on
 * the device in a fixed order (the same bits on every run) and mergeable: chunks, batches and
 * ranks combine through twosd_moments_merge, so a shard layout fixes the bits.
 * variance = m2 / (n - 1); standard error of the mean = sqrt(variance / n).
 */
typedef struct twosd_moments {
    int64_t n;      /* scenarios counted: LP optimal                                    */
    int64_t n_bad;  /* scenarios left out: LP not optimal                               */
    double mean;    /* of obj over the n            (0 when n == 0)                     */
    double m2;      /* sum (obj - mean)^2 over them (0 when n <= 1)                     */
    double min, max;/* +inf / -inf when n == 0                                          */
} twosd_moments;

/* out = a merged with b (host code only: no context, no GPU call; out may alias a or b).  With
 * n = na + nb and d = mean_b - mean_a: mean = mean_a + d (nb / n), m2 = m2_a + m2_b + d d (na nb / n);
 * n_bad adds.  An operand with n == 0 gives the other operand's fields bit for bit (n_bad added). */
int twosd_moments_merge(const twosd_moments *a, const twosd_moments *b, twosd_moments *out);

/* Moments of the caller's own objectives obj[n]; status[n] nullable (every entry counts), else
 * only entries with TWOSD_LP_OPTIMAL count and the others' values are never read into a sum
 * (they may be NaN).  Uploads the arrays and runs the moments kernel; needs no template. */
int twosd_moments_of_values(twosd_ctx *ctx, int64_t n, const double *obj, const int *status, twosd_moments *out);

/* Moments of the stage-2 objective at x over scenarios [first, first+count) of stream `seed`
 * (the scenarios of twosd_evaluate_sampled): per chunk of 2^20 scenarios sample, solve, reduce on
 * the device -- no objective is copied to the host; chunks merge in ascending order.  A
 * non-optimal LP does not abort: the scenario counts in n_bad, *out is filled and the return
 * value is TWOSD_E_LP.  The caller adds c'x to the mean. */
int twosd_evaluate_moments(twosd_ctx *ctx, const double *x, int64_t first, int64_t count, uint64_t seed,
                           twosd_moments *out);

/* Two first-stage points on common random numbers: the same scenarios solved at xa and at xb.  A
 * scenario counts when its LP is optimal at both (a->n == b->n == diff->n); *diff holds the
 * moments of obj(xa) - obj(xb) formed per scenario.  Outputs and return value as above. */
int twosd_evaluate_paired(twosd_ctx *ctx, const double *xa, const double *xb, int64_t first, int64_t count,
                          uint64_t seed, twosd_moments *a, twosd_moments *b, twosd_moments *diff);

/* Sample until the confidence interval is tight: batch j is scenarios [first + j batch, ...) of
 * the stream, merged in order.  After each batch with n >= 2: hw = z sqrt(m2 / (n - 1) / n);
 * stops with *converged = 1 when hw <= max(abs_tol, rel_tol |offset + mean|), or with
 * *converged = 0 once n + n_bad >= n_max (the last batch is clipped to n_max).  offset is the
 * caller's c'x; z a normal quantile (1.96 for 95 %).  *half_width = +inf while n < 2.
 * TWOSD_E_ARG for batch < 2, n_max < batch, z <= 0 or a negative tolerance. */
int twosd_evaluate_ci(twosd_ctx *ctx, const double *x, uint64_t seed, int64_t first, int64_t batch, int64_t n_max,
                      double z, double rel_tol, double abs_tol, double offset, twosd_moments *out,
                      double *half_width, int *converged);

/*
 * The estimators above on a variance-reduced stream (twosd_sampling).  The members of a group
 * are dependent, so the observations are the GROUP MEANS: in every twosd_moments these calls
 * return, n and n_bad count groups (a group counts only if all G of its LPs are optimal; the
 * values of a group left out are never read into a sum), and mean, m2, min and max are of group
 * means.  The scenarios behind a record are G (n + n_bad).  The mean of a group v[0 .. G) is
 * K + (sum_{i = 0 .. G-1} (v[i] - K)) / G with K = v[0], the sum taken in index order from 0.0,
 * every operation rounded to nearest, no fused multiply-add -- the same bits under any launch
 * shape.  The moments of the means are those of twosd_moments_of_values, taken per chunk on
 * m_b - K0 with K0 = the chunk's entry 0 (0 when that entry is not optimal or not finite) and K0
 * added back to mean, min and max: the records merge at the size of the spread, and min / max are
 * the means' own bits whenever m_b / 2 <= K0 <= 2 m_b.  A NULL plan or G = 1 is the namesake call
 * itself.
 *   moments_of_values_grouped: the caller's obj[n] / status[n] (nullable) in groups of G,
 *     1 <= G <= 256; TWOSD_E_ARG unless n is a multiple of G.
 *   evaluate_moments_vr / _paired_vr: first and count multiples of G.  The chunk of 2^20
 *     scenarios is rounded down to a multiple of G.  Paired: a and b are reduced to group means and
 *     diff holds the moments of mean_a - mean_b per group.
 *   evaluate_ci_vr: first and batch multiples of G with batch / G >= 2; n_max is clipped down to
 *     a multiple of G (TWOSD_E_ARG if that leaves less than batch).  The stop rule is
 *     twosd_evaluate_ci's on the group moments: hw = z sqrt(m2 / (n - 1) / n), n in groups.
 */
int twosd_moments_of_values_grouped(twosd_ctx *ctx, int64_t n, int G, const double *obj, const int *status,
                                    twosd_moments *out);
int twosd_evaluate_moments_vr(twosd_ctx *ctx, const double *x, int64_t first, int64_t count, uint64_t seed,
                              twosd_moments *out, const twosd_sampling *plan);
int twosd_evaluate_paired_vr(twosd_ctx *ctx, const double *xa, const double *xb, int64_t first, int64_t count,
                             uint64_t seed, twosd_moments *a, twosd_moments *b, twosd_moments *diff,
                             const twosd_sampling *plan);
int twosd_evaluate_ci_vr(twosd_ctx *ctx, const double *x, uint64_t seed, int64_t first, int64_t batch, int64_t n_max,
                         double z, double rel_tol, double abs_tol, double offset, twosd_moments *out,
                         double *half_width, int *converged, const twosd_sampling *plan);

/*
 * solve_problem! (smps_routines.jl:50-62) for scenarios [first, first+count) of epigraph
 * `epi` at first-stage x[n1].  obj[count], status[count] required; pi[count*m2] and
 * y[count*n2] nullable.  Returns TWOSD_E_LP if any status != OPTIMAL (outputs still set).
 */
int twosd_solve_batch(twosd_ctx *ctx, int epi, const double *x, int first, int count,
                      double *obj, double *pi, double *y, int *status);

/* Same for scenarios given by value (evaluate(), smps_routines.jl:67-82): values[N*k]. */
int twosd_solve_values(twosd_ctx *ctx, const double *x, int N, const double *values,
                       double *obj, double *pi, double *y, int *status);

/*
 * push!(::sdDualVertexSet, pi) batched (dual_set.jl:84-94): pis[count*m2] are pushed in
 * order; out_index[count] (nullable) receives the 0-based vertex index each one maps to;
 * *new_size the set size afterwards.  Exact reference dedup semantics: 16-significant-bit
 * L1 hash + component-wise 16-bit rounding compare, first occurrence kept.
 */
int twosd_dvs_push(twosd_ctx *ctx, int count, const double *pis, int *out_index, int *new_size);
int twosd_dvs_size(twosd_ctx *ctx, int *size);
int twosd_dvs_get(twosd_ctx *ctx, int first, int count, double *out /* count*m2 */);
int twosd_dvs_clear(twosd_ctx *ctx);
/* Truncate the set to its first `size` vertices (rollback of a speculative push). */
int twosd_dvs_truncate(twosd_ctx *ctx, int size);
/* Order-dependent 64-bit digest of the set (size and the per-vertex dedup fingerprints in
 * insertion order).  No reference counterpart: ranks compare it so that a cut all-reduce
 * over vertex indices only runs on identical ordered sets (the reference is single-process,
 * cell.jl:25 shares one set). */
int twosd_dvs_fingerprint(twosd_ctx *ctx, uint64_t *digest);

/*
 * sd_iteration! hot segment for one epigraph (algorithm.jl:45-55): solve scenarios
 * [first, first+count) at x and push their duals into the vertex set on the device
 * (no host round trip).  obj/status nullable.
 */
int twosd_solve_push(twosd_ctx *ctx, int epi, const double *x, int first, int count,
                     double *obj, int *status, int *new_size);
/* Scenarios whose dual the last twosd_solve_push recovered and pushed: the first scenario of
 * each distinct optimal dual vertex of the batch (every later scenario at a vertex pushes an
 * equal vector, a no-op of push!, dual_set.jl:84-94); `count` with TWOSD_PUSH_ALL=1. */
int twosd_last_push_reps(twosd_ctx *ctx, int *reps);
/* How the last twosd_solve_push obtained the representatives' duals: 0 = re-solved with dual
 * recovery after the keyed main pass; 1 = recovered for every scenario in the main pass and
 * gathered (chosen when the previous keyed push re-solved more than a quarter of its batch;
 * TWOSD_PUSH_MODE=1 / 2 forces one or the other).  The pushed rows are the same either way. */
int twosd_last_push_mode(twosd_ctx *ctx, int *full);

/*
 * build_sasa_cut (epigraph.jl:125-146) incl. argmax_procedure (subprob.jl:141-169) over
 * every scenario of epigraph `epi` and the current vertex set, at x:
 *   alpha, beta[n1], weight_mark (= total scenario weight); max_val[N], max_arg[N]
 *   (0-based vertex index) nullable.  Ties: lowest vertex index among scores within
 *   tie_rel*(1+|max|) of the maximum (tie_rel = 0 -> strict '>' as the reference).
 */
int twosd_build_cut(twosd_ctx *ctx, int epi, const double *x, double tie_rel,
                    double *alpha, double *beta, double *weight_mark,
                    double *max_val, int *max_arg);

/*
 * Counters of the last twosd_build_cut / twosd_cut_partial (diagnostics, synchronous read):
 * out[0] scenarios re-decided in the restatement's arithmetic (several vertices within the
 * MFMA scores' error band of the maximum), out[1] candidate vertices scored for them, out[2]
 * scenarios re-scanned over every vertex (a candidate log overflowed), out[3] vertices left out
 * of the argmax as dominated twins (a lower vertex with a bit-identical PK row and an equal base
 * at this x: never the pick under either tie rule).  out has 4 entries.
 */
int twosd_cut_stats(twosd_ctx *ctx, int64_t *out);

/*
 * The MFMA pass the last twosd_build_cut / twosd_cut_partial ran (diagnostics, synchronous read):
 * *fp32 = 1 the fp32 pass (v_mfma_f32_16x16x4f32, decisions within its wider error band), 0 the
 * fp64 pass (TWOSD_CUT_F32=0, or operands outside the fp32 envelope); *band = that pass's
 * decision band.  Either pass gives the restatement's picks (cut_fixup_kernel re-decides every
 * row with several vertices in the band).
 */
int twosd_cut_pass(twosd_ctx *ctx, int *fp32, double *band);

/*
 * Which pass that was: *kind = 0 the fp64 MFMA pass, 1 the fp32 one, 2 the integer one
 * (v_mfma_i32_16x16x64_i8 over int8 limbs of fixed-point operands: exact int32 sums, the only error
 * the bounded operand quantisation; sqlp_amd/csrc/cut_i8.h).  twosd_cut_pass reports *fp32 = 1 for
 * kinds 1 and 2 and the band of the pass that ran.  *limbs / *pairs (may be NULL): the integer
 * pass's build-time limb count and number of kept limb pairs.  The integer pass is the default
 * reduced-precision pass; TWOSD_CUT_I8=0 selects the fp32 one, TWOSD_CUT_F32=0 the fp64 one, and
 * the device falls back by itself (fp32 envelope failed: 0; a NaN or infinite delta seen: 1).
 */
int twosd_cut_pass_kind(twosd_ctx *ctx, int *kind, int *limbs, int *pairs);

/*
 * Diagnostics for tests: runs one cut of epigraph epi at x (tie_rel 0) and writes the integer
 * pass's score term t (fp32; the score is base[v] + t) of every scenario s and compacted vertex
 * position c to out[s * nvc + c], computed by the pass's own device functions.  *nvc_out = the
 * number of compacted vertices, vmap_out (may be NULL, |V| entries) their vertex indices.  Limited to
 * N |V| <= 2^20; cap = the floats out holds.  TWOSD_E_STATE when the integer pass is switched off.
 */
int twosd_cut_debug_scores(twosd_ctx *ctx, int epi, const double *x, float *out, int64_t cap, int *nvc_out,
                           int *vmap_out);

/*
 * Multi-GPU split of twosd_build_cut: each rank computes partial sums over its own
 * scenarios into a caller-provided DEVICE buffer (layout in twosd_cut_partial_len),
 * the caller all-reduces it (sum; e.g. torch.distributed / RCCL), then finalize.
 * The partial holds the vertex weight histogram as uint64 fixed point (exact, order
 * independent) followed by fp64 sums.  total_weight is the global total scenario weight.
 */
int twosd_cut_partial_len(twosd_ctx *ctx, int64_t *n_u64, int64_t *n_f64);
int twosd_cut_partial(twosd_ctx *ctx, int epi, const double *x, double tie_rel, double total_weight,
                      uint64_t *d_hist_u64, double *d_sums_f64, double *max_val, int *max_arg);
int twosd_cut_finalize(twosd_ctx *ctx, const double *x, const uint64_t *d_hist_u64, const double *d_sums_f64,
                       double *alpha, double *beta);

/*
 * Stored picks (no reference counterpart: the reference's readme lists "Need to implement
 * stopping criteria" and src/sd_algorithm/plugin/stopping_rule.jl is an empty file).  With its
 * argmax picks fixed, a cut is a linear function of the scenario weights, so the in-sample
 * stopping rule of SD re-forms cuts under resampled weights without repeating the argmax.
 *   picks_keep: snapshot the picks of the last twosd_build_cut / twosd_cut_partial of epigraph epi
 *     (a device-to-device copy on the context's stream, no host round trip) with the scenario
 *     count n and |V| = nv of that cut.  A handle costs 4 bytes per scenario of device memory.
 *     TWOSD_E_STATE if the last cut call was not for epi, took the empty-epigraph path, or the
 *     template, the positions or the vertex set were reset since.
 *   picks_info / picks_get (out[n], 0-based vertex indices) / picks_release; picks_count: live handles.
 * twosd_set_template, twosd_set_random_positions and twosd_destroy drop every handle.  After
 * twosd_dvs_clear / twosd_dvs_truncate a handle whose nv exceeds the new size is unusable
 * (TWOSD_E_STATE on use; release it).  Scenario rows are append-only, so a handle stays valid while
 * its epigraph grows: it covers the first n scenarios.
 */
int twosd_picks_keep(twosd_ctx *ctx, int epi, int *handle);
int twosd_picks_info(twosd_ctx *ctx, int handle, int *epi, int *n, int *nv);
int twosd_picks_get(twosd_ctx *ctx, int handle, int *out);
int twosd_picks_release(twosd_ctx *ctx, int handle);
int twosd_picks_count(twosd_ctx *ctx, int *live);

/*
 * Bootstrap replicate counts (no reference counterpart: plugin/stopping_rule.jl is empty).
 * Replicate b (0 <= b < M) gives the scenario with global index g (as in the sampler) the count
 * c_b(g), an independent Poisson(1) draw and a pure function of (seed, g, b): Philox4x32-10 with
 * counter (g_lo, g_hi, b >> 2, 1) and key (seed_lo, seed_hi) -- the last counter word keeps the
 * stream apart from the scenario stream, which uses 0 -- whose output word b & 3 is u, and
 * c = #{ j : u >= T_j } over T_j = round-half-even(2^32 sum_{i<=j} e^-1 / i!), j = 0..11:
 *   0x5e2d58d9 0xbc5ab1b1 0xeb715e1e 0xfb239797 0xff1025f6 0xffd90f3c
 *   0xfffa8b72 0xffff540c 0xffffed1f 0xfffffe21 0xffffffd5 0xfffffffc
 * (counts 0..12).  count_of_word: host code only, no context.  bootstrap_counts: the device draw
 * of scenarios [first_index, first_index + count), out[s * M + b]; 1 <= M <= 64, count <= 2^24.
 */
int twosd_bootstrap_count_of_word(uint32_t u);
int twosd_bootstrap_counts(twosd_ctx *ctx, int M, uint64_t seed, uint64_t first_index, int64_t count, uint8_t *out);

/*
 * The bootstrap on a variance-reduced epigraph (twosd_sampling, group G): the observations of such
 * a stream are its groups, so the bootstrap resamples whole groups.  The count of the scenario with
 * global index g in replicate b is c_b(g / G): the count function above, indexed by the GLOBAL GROUP
 * INDEX.  Every member of a group carries its group's count and keeps its own weight w_s; integer
 * weights, the normalisation by the replicate's own W_jb, the identity row 0 and the zero cut at
 * W_jb = 0 are those of twosd_reform_cuts.  G = 1 (a NULL plan or mode IID) is the namesake call
 * itself, bit for bit.  Sharding on group boundaries reproduces the draws.
 *   bootstrap_counts_vr: first_index and count multiples of G; out[s * M + b] = c_b((first_index + s) / G).
 *   reform_cuts_vr / reform_partial_vr: index_offset, the epigraph's current scenario count and every
 *     handle's N_j multiples of G.  twosd_reform_partial_len and twosd_reform_finalize do not depend
 *     on the plan.
 * TWOSD_E_ARG with the offending value in the message for an invalid plan (as every _vr call) and
 * for each quantity above that is not in whole groups (a handle is named).
 */
int twosd_bootstrap_counts_vr(twosd_ctx *ctx, int M, uint64_t seed, uint64_t first_index, int64_t count, uint8_t *out,
                              const twosd_sampling *plan);

/*
 * Re-formed cuts under bootstrap weights (the device part of the in-sample stopping rule; no
 * reference counterpart: plugin/stopping_rule.jl is empty).  For each of the H handles (all of
 * epigraph epi) and each row b of M + 1 -- row 0 the identity replicate (all counts 1), row 1 + b
 * replicate b -- with c(s) the count of scenario index_offset + s and N_j the handle's scenarios:
 *     W_jb = sum_{s < N_j} c(s) w_s,   p_s = c(s) w_s / W_jb,
 *     g = sum_s p_s pi_pick(s),  S_e = sum_s p_s PK[pick(s), e] dv[s, e],
 *     alpha = g.r + sum_{e rhs} S_e (+ c0 once for a template with general bounds),
 *     beta = -T'g - sum_{e in T} S_e e_col(e),   weight_mark = W_jb
 * (build_sasa_cut's formula, epigraph.jl:125-146, with the picks fixed; dual vectors of length mv).
 * W_jb = 0 gives the zero cut with weight_mark 0, the reference's empty-epigraph cut.
 * total_weight[b] = sum_{s < N} c(s) w_s over all scenarios the epigraph holds now.
 * Outputs (host): alpha[b * H + j], beta[(b * H + j) * n1 + i], weight_mark[b * H + j] (nullable),
 * total_weight[M + 1] (nullable).  Row 0 equals the cut twosd_build_cut returned up to rounding.
 * Weights are summed as integers (w 2^58 / total weight, rounded), so weight_mark and
 * total_weight carry a relative error of at most N 2^-59 total / W and are the same bits on
 * every run; the fp64 sums use a fixed shard layout (the same bits on every run, and the same
 * for H handles in one call as in H calls).
 * TWOSD_E_ARG unless 0 <= M <= 64 (M = 0: the identity row alone), H >= 1 and every handle
 * belongs to epi; TWOSD_E_UNSUPPORTED for k beyond the cut envelope of 127.
 *
 * Multi-GPU split, as twosd_cut_partial_len / _partial / _finalize: each rank runs reform_partial
 * over its own scenarios (index_offset = the global index of its first one; its handles mirror the
 * other ranks', vertex sets identical) into caller DEVICE buffers of *n_u64 uint64 (the totals,
 * the W_jb and the per-vertex weights: integers, exact under any order of summation) and *n_f64
 * doubles (the unnormalised S_e); the caller sums them over the ranks and every rank finalizes.
 * total_weight: the GLOBAL total scenario weight of the epigraph, the same value on every rank
 * (it fixes the integer scale).  twosd_reform_cuts is partial then finalize on one context.
 */
int twosd_reform_cuts(twosd_ctx *ctx, int epi, int H, const int *handles, int M, uint64_t seed, uint64_t index_offset,
                      double *alpha, double *beta, double *weight_mark, double *total_weight);
int twosd_reform_partial_len(twosd_ctx *ctx, int H, const int *handles, int M, int64_t *n_u64, int64_t *n_f64);
int twosd_reform_partial(twosd_ctx *ctx, int epi, int H, const int *handles, int M, uint64_t seed, uint64_t index_offset,
                         double total_weight, uint64_t *d_u64, double *d_f64);
int twosd_reform_finalize(twosd_ctx *ctx, int H, const int *handles, int M, double total_weight, const uint64_t *d_u64,
                          const double *d_f64, double *alpha, double *beta, double *weight_mark, double *total_weight_out);
/* The same under a sampling plan: whole groups are resampled (see twosd_bootstrap_counts_vr). */
int twosd_reform_cuts_vr(twosd_ctx *ctx, int epi, int H, const int *handles, int M, uint64_t seed, uint64_t index_offset,
                         double *alpha, double *beta, double *weight_mark, double *total_weight, const twosd_sampling *plan);
int twosd_reform_partial_vr(twosd_ctx *ctx, int epi, int H, const int *handles, int M, uint64_t seed, uint64_t index_offset,
                            double total_weight, uint64_t *d_u64, double *d_f64, const twosd_sampling *plan);
/* Device time of the last twosd_reform_cuts on the context's stream (HIP events), milliseconds:
 * [0] the partial sums (histograms, delta streaming, reductions), [1] the finalize with its copies. */
int twosd_reform_last_ms(twosd_ctx *ctx, double *ms2);

/* ---- risk measures: weighted quantiles, tail cuts, out-of-sample CVaR -----
 * No reference counterpart: the reference optimises the expectation only.  Mean-CVaR in the form
 * of Rockafellar and Uryasev, CVaR_a(h) = min_eta eta + E[(h - eta)+] / (1 - a).
 *
 * twosd_quantile_of_values: VaR and CVaR at `level` of the caller's own n values (1 <= n <= 2^27),
 * selected on the device.  An entry counts when status is NULL or its status is TWOSD_LP_OPTIMAL;
 * the others are counted in *n_bad and their values are never read into a sum (they may be NaN).
 * Weights are integers: q_s = rn(w_s * rn(2^58 / W)) with W the weights' sum in index order (the
 * scale of twosd_reform_cuts), or q_s = 1 when weights is NULL.  With Q = sum q_s over the counted
 * entries and t = ceil(level * Q), taken exactly (level is a dyadic rational):
 *     *var     = the smallest counted value v with sum_{value <= v} q_s >= t,
 *     *tail_q  = sum_{value > *var} q_s,   *total_q = Q   (integers: the same bits on every run),
 *     *cvar    = *var + (sum_{value > *var} q_s (value_s - *var)) / ((1 - level) Q).
 * Values are ordered by their sign-flipped bit patterns: the numeric order, with -0 before +0.  The
 * fp64 sum has a fixed shard layout and every operation is rounded on its own, so all outputs are
 * bit-identical on every run and under any launch grid.  Every output is nullable.
 * TWOSD_E_ARG unless 0 < level < 1, 1 <= n <= 2^27, every weight is finite and >= 0, and some
 * entry counts with a positive integer weight (*n_bad and *total_q are still set then).
 *
 * twosd_cut_quantile: the same over the last cut of epigraph epi -- the values are its scenarios'
 * maximal scores in the caller's space (val[s] + c0 in one rounded add: what twosd_build_cut
 * returns in max_val), the weights the scenario weights with W the epigraph's total weight.
 * *tail_weight and *total_weight are tail_q and Q times W / 2^58.  The state rule is that of
 * twosd_picks_keep: TWOSD_E_STATE if the last cut call was not for epi, took the empty-epigraph
 * path, or the template, the positions or the vertex set were reset since.
 *
 * twosd_cut_tail: the tail cut of the last cut of epi at eta (same state rule).  With
 * f_s = 1[(val[s] + c0) > eta] (strict; the rounded sum above) and a(s) the stored pick:
 *     W_t = sum f_s w_s,   p_s = f_s w_s / W_t,
 *     g = sum p_s pi_a(s),   S_e = sum p_s PK[a(s), e] dv[s, e],
 *     *alpha = g.r + sum_{e rhs} S_e + c0,   beta = -T'g - sum_{e in T} S_e e_col(e)    (beta: n1)
 * -- twosd_reform_cuts with the counts f, its integer weights and fixed shard layout (bit-identical
 * on every run and under any grid).  *tail_weight = W_t and *total_weight = the weight of the cut's
 * scenarios, both through the integer scale (nullable).  No scenario in the tail: the zero cut with
 * *tail_weight = 0.  With d = *tail_weight / *total_weight the row
 *     tau >= d (alpha + beta'x - eta)
 * is a subgradient of (1/W) sum_s w_s (max_v pi_v (r_s - T_s x) - eta)+ at the cut's x and eta, so
 * it bounds the sample's E[(h - eta)+] from below at every (x, eta).
 * TWOSD_E_UNSUPPORTED for k beyond the cut's envelope of 127; TWOSD_E_ARG for a NaN eta.
 *
 * twosd_risk_last_ms: device time (HIP events, milliseconds) of [0] the last quantile selection
 * (of any of the calls here) and [1] the last twosd_cut_tail, copies included. */
int twosd_quantile_of_values(twosd_ctx *ctx, int64_t n, const double *values, const double *weights, const int *status,
                             double level, double *var, double *cvar, uint64_t *tail_q, uint64_t *total_q, int64_t *n_bad);
int twosd_cut_quantile(twosd_ctx *ctx, int epi, double level, double *var, double *cvar, double *tail_weight,
                       double *total_weight);
int twosd_cut_tail(twosd_ctx *ctx, int epi, double eta, double *alpha, double *beta, double *tail_weight,
                   double *total_weight);
int twosd_risk_last_ms(twosd_ctx *ctx, double *ms2);

/*
 * Tail handles: the tail of the last cut of epi at eta as a compact list, so that a tail row can be
 * re-formed under resampled weights (the stopping rule of the mean-CVaR loop).  With its tail set
 * and picks fixed a tail row is linear in the scenario weights, as a mean cut is; at the (x, eta) it
 * was built at the re-formed row is the replicate's own E_b[(h - eta)+] (the set {h_s > eta} does
 * not depend on the weights), and a fixed set bounds it from below everywhere else.
 *   tail_keep: the nt scenarios s of the cut with f_s = 1[(val[s] + c0) > eta] -- twosd_cut_tail's
 *     flag bit for bit, the set it sums over -- in ascending order, and their picks.  State rule and
 *     refusals of twosd_cut_tail (TWOSD_E_ARG for a NaN eta, TWOSD_E_UNSUPPORTED for k > 127).  The
 *     list is compacted on the device (per 64-scenario tile a ballot of the flags, an exclusive scan
 *     of the tiles' counts, a scatter by offset plus lane rank: the same under any grid); no score or
 *     pick leaves the device, nt alone is copied to size the arrays.  A handle costs 8 bytes per TAIL
 *     scenario.  nt = 0 (eta at or above every score) is a valid handle.
 *   tail_info: the cut's (epi, n, nv), nt and eta (each nullable); tail_get: scen[nt], pick[nt].
 *   tail_last_ms: device time of the last twosd_tail_keep (HIP events, milliseconds).
 * Tail handles live in the pick handles' table: twosd_picks_info reports (epi, n, nv) of the cut,
 * twosd_picks_release and twosd_picks_count cover them, the calls that drop or disable pick handles
 * do the same to them; twosd_picks_get refuses one (TWOSD_E_ARG: use twosd_tail_get) and the tail_
 * calls refuse a pick handle.
 *
 * twosd_reform_cuts, _partial, _partial_len, _finalize and their _vr forms take tail handles mixed
 * freely with pick handles of the same epigraph.  For a tail handle j the counts are c_b(s) f_s:
 *     W_jb = sum_{i < nt} c_b(scen_i) w_{scen_i},  alpha, beta: the formula above over the list,
 *     weight_mark = W_jb;   W_jb = 0 or nt = 0: the zero cut with weight_mark 0
 * -- the count of an entry is that of its scenario's global index index_offset + scen_i (of its group
 * under a plan), so the row is the one a pick handle with -1 outside the tail would give.  Only the
 * tail's deltas are read: three kernels over the list, shards = those of nt entries, summed as every
 * handle's (the same bits on every run, and for H handles in one call as in H calls); nothing is
 * launched over an empty list.  The handle's words of the partial buffers stay what they are.
 */
int twosd_tail_keep(twosd_ctx *ctx, int epi, double eta, int *handle);
int twosd_tail_info(twosd_ctx *ctx, int handle, int *epi, int *n, int *nv, int *nt, double *eta);
int twosd_tail_get(twosd_ctx *ctx, int handle, int *scen, int *pick);
int twosd_tail_last_ms(twosd_ctx *ctx, double *ms);

/* Out-of-sample CVaR of the stage-2 objective at x over scenarios [first, first + count) of the
 * i.i.d. device stream `seed` (1 <= count <= 2^27; TWOSD_E_UNSUPPORTED beyond): sampled and solved
 * in the chunks of twosd_evaluate_moments, the objectives and statuses of the whole range kept on
 * the device (12 bytes per scenario) and never copied to the host.  var = the level-quantile with
 * unit weights (twosd_quantile_of_values); y = the moments, reduced once over the whole range, of
 *     Y_s = var + max(obj_s - var, 0) / (1 - level)        (each operation rounded on its own)
 * so cvar = y.mean and sqrt(y.m2 / (n - 1) / n) is its asymptotic standard error (the plain-sample
 * one: the quantile's own estimation error enters in second order only).  n / n_bad: optimal and
 * other LPs; with n_bad > 0 the return value is TWOSD_E_LP and *out is filled from the optimal
 * ones.  The caller adds c'x to var and cvar.  There is no plan argument: i.i.d. streams only. */
typedef struct twosd_cvar {
    int64_t n, n_bad;
    double var, cvar;
    twosd_moments y;
} twosd_cvar;
int twosd_evaluate_cvar(twosd_ctx *ctx, const double *x, uint64_t seed, int64_t first, int64_t count, double level,
                        twosd_cvar *out);

/* Timing of the last kernel phases on the context's stream (HIP events), microseconds:
 * [0] LP kernel, [1] dedup push, [2] argmax+cut partial, [3] cut finalize,
 * [4] warm-start pool selection of the last LP batch (0 without a pool). */
int twosd_last_timings(twosd_ctx *ctx, double *us5);

/* Statistics of the last LP batch: sum of simplex pivots, max pivots. */
int twosd_last_lp_stats(twosd_ctx *ctx, int64_t *pivots_sum, int *pivots_max);
/* Eta-file entries the last LP batch wrote to the per-wavefront eta arena (12 bytes each: row index
 * and value), summed over its scenarios: the algorithmic share of the LP kernel's HBM writes.
 * *retries (nullable): its scenarios whose pool start ended non-optimal (iteration cap, numerics)
 * and were solved again from the primary basis. */
int twosd_last_lp_eta_entries(twosd_ctx *ctx, int64_t *entries, int64_t *retries);

/* Incumbent objective of the last twosd_solve_batch / twosd_solve_push / twosd_solve_values
 * batch: *weighted_sum = sum_s w_s obj_s and *weight_sum = sum_s w_s over its scenarios (the
 * epigraph's add_scenario! weights; 1.0 for solve_values), reduced in a fixed order (the same
 * bits on every run).  weighted_sum / weight_sum is the sample-average recourse at x that
 * evaluate (smps_routines.jl:67-82) and the incumbent estimate of sd_iteration! form; across
 * ranks the caller adds the ranks' sums (north star: the all-reduce of the incumbent objective). */
int twosd_last_objective(twosd_ctx *ctx, double *weighted_sum, double *weight_sum);

/* Diagnostic: pivots and status of every scenario of the last LP launch (by scenario index;
 * after a pool refresh: its training solves). */
int twosd_last_lp_iters(twosd_ctx *ctx, int N, int *iters, int *status);

/* Pivot cap of the training solves of a pool refresh: > 0 explicit, 0 auto (default: 3 x the
 * mean pivots of the last batch of >= 4096 scenarios, at least 32; none before such a batch),
 * < 0 none (the kernel's kmax).  A training scenario that needs more pivots drops out of the
 * basis count instead of holding the launch: one wavefront per scenario, so a launch lasts as
 * long as its slowest scenario. */
int twosd_set_refresh_kcap(twosd_ctx *ctx, int kcap);

/* Executed fp64 row operations of the last LP batch: each is one fused multiply-add over
 * a padded basis row of *row_width (= 64 * ceil(m2/64)) doubles, i.e. 2 * row_width flops
 * (used for the counted-FLOP roofline of the LP kernel). */
int twosd_last_lp_ops(twosd_ctx *ctx, int64_t *row_ops, int *row_width);

/* Diagnostic: per-phase cycle totals of the hypersparse LP kernel, summed over waves
 * (non-zero only in the TWOSD_STAMPS build libtwosd_hip_stamps.so).  reset != 0 clears. */
int twosd_debug_stamps(twosd_ctx *ctx, uint64_t *out10, int reset);

/* ---- feasibility rays --------------------------------------------------
 * A ray sigma (mv = m_lp doubles, bound rows included) has the sign convention of a dual:
 * sigma_i >= 0 on G rows, <= 0 on L rows (bound rows are L), free on E rows; sigma' W_j <= 0 for
 * every structural column (to the ratio test's pivot tolerance); sigma' b > 0 certifies that the LP
 * with right-hand side b = [r_w - T_w x - W s ; hi - lo] has no solution.  W is not random, so a
 * ray found at one scenario certifies every scenario and every x with sigma' b_w(x) > 0.
 *
 * The ray set F of a context: at most TWOSD_FRAY_MAX rays, normalised (divided by max |sigma_i|
 * after the entries at or below 1e-12 (1 + max) are set to zero), in insertion order.  A pushed ray
 * whose key is present maps to the existing index (first occurrence kept); the key is the
 * components rounded to 24 significant bits, mixed with their row.  twosd_fray_push: rays[count*mv]
 * in order, out_index[count] (nullable), *new_size (nullable).  TWOSD_E_ARG when a ray is all zero
 * or not finite, TWOSD_E_UNSUPPORTED when the set would pass TWOSD_FRAY_MAX; either leaves the set
 * as it was.  The set is dropped by twosd_set_template and twosd_set_random_positions.
 * twosd_fray_key is a pure host function (no context, no GPU call): the key and the normalised
 * form (each nullable) of one ray, exactly what a push computes. */
#define TWOSD_FRAY_MAX 4096
int twosd_fray_push(twosd_ctx *ctx, int count, const double *rays, int *out_index, int *new_size);
int twosd_fray_size(twosd_ctx *ctx, int *size);
int twosd_fray_get(twosd_ctx *ctx, int first, int count, double *out /* count*mv */);
int twosd_fray_clear(twosd_ctx *ctx);
int twosd_fray_key(const double *ray, int mv, uint64_t *key, double *normalised /* mv */);

/* Solve scenarios [first, first+count) of epigraph `epi` at x as twosd_solve_batch does without
 * outputs, then recover one Farkas ray per distinct infeasible exit: the infeasible scenarios are
 * compacted (ascending) and re-solved from their recorded start bases, 4096 at a time, by the LP
 * kernel's ray instantiation; of every (final basis, leaving variable, sign) the first scenario's
 * ray is kept, in scenario order, until `cap` rays.  *n_infeasible = infeasible scenarios,
 * *n_rays = rays returned; scen[i] (cap) = the scenario of ray i as an index of the epigraph;
 * rays (cap*mv, nullable) raw (unnormalised) sigma = +-e_r' B^{-1}; row (cap, nullable) the leaving
 * row r (a basis position); head (cap*m_lp, nullable) the basis at the exit (column j < n_lp, or
 * n_lp + i for the slack of row i); status (count, nullable).  push != 0 also pushes the returned
 * rays into F on the device.  TWOSD_OK when every scenario is optimal or infeasible; TWOSD_E_LP
 * only when one ended at the iteration limit or numerically; TWOSD_E_ARG / TWOSD_E_STATE as
 * twosd_solve_batch.  A batch without an infeasible scenario launches what twosd_solve_batch
 * launches. */
int twosd_solve_rays(twosd_ctx *ctx, int epi, const double *x, int first, int count, int cap, int push,
                     int *n_infeasible, int *n_rays, int *scen, double *rays, int *row, int *head, int *status);
/* Of the last twosd_solve_rays: list positions the ray instantiation re-solved, and infeasible
 * scenarios it did not have to because a ray held or found before their chunk cuts them off at x
 * (the violation scan runs over the remaining list before every chunk after the first, and before
 * the first when F is not empty); *scan_us: device time (events) of the scan and merge kernels of
 * the last twosd_feas_scan, in microseconds.  Each nullable. */
int twosd_last_ray_stats(twosd_ctx *ctx, int64_t *resolved, int64_t *filtered, double *scan_us);

/* Violation scan of scenarios [first, first+count) (count >= 1) of epigraph `epi` against every ray
 * of F at x.  The score of (ray j, scenario s) is v_js = alpha + beta' x of their feasibility row
 *     alpha = sigma . [ r_w - W s ; hi - lo ],   beta = -T_w' sigma      (alpha + beta' x <= 0)
 * evaluated in the arithmetic of the cut's restated score: sigma_j . (r - T x) in index order plus
 * the random elements' terms by ascending row, every product and sum rounded on its own.
 * ray_max[J] = max_s v_js and ray_arg[J] the lowest scenario index (of the epigraph) attaining it;
 * alpha[J] / beta[J*n1] (each nullable) the row of (j, ray_arg[j]); cut_off[count] (nullable) whether
 * any ray scores > 0 at the scenario, *n_cut_off (nullable) their number.  Bit-identical under any
 * launch grid.  TWOSD_E_STATE when F is empty; TWOSD_E_UNSUPPORTED for k beyond the cut's 127. */
int twosd_feas_scan(twosd_ctx *ctx, int epi, const double *x, int first, int count, double *ray_max, int *ray_arg,
                    double *alpha, double *beta, int64_t *n_cut_off, unsigned char *cut_off);

#ifdef __cplusplus
}
#endif
#endif /* TWOSD_HIP_H */
