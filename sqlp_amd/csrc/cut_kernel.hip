// cut_kernel.hip -- argmax_procedure + build_sasa_cut on gfx950 (fp64 MFMA).
//
// Reference: argmax_procedure (src/sd_algorithm/subprob.jl:141-169) and build_sasa_cut
// (src/sd_algorithm/epigraph.jl:125-146).  For scenario w (element deltas dv[w,e] at
// rows row_e; coef_e = 1 for an RHS element, -x[col_e] for a T element):
//     score[w,v] = pi_v . (r - T x)  +  sum_e pi_v[row_e] * coef_e * dv[w,e]
//                = base[v]          +  (DR_w . PK_v)           (an N x |V| x k GEMM)
//     a(w)  = lowest v within tie_rel*(1+|max|) of max_v score[w,v]   (tie_rel=0: the
//             reference's strict '>' first maximum)
// The DECISION is made on scores evaluated in the restatement's arithmetic order
// (oracle/cpu_lp.c oracle_build_cut; subprob.jl:147-158 with the dots sequential, no
// contraction): base[v] = sum_i pi_v[i] * bvec[i] in index order, then
// score = base[v] + (sum_e pi_v[row_e] * (coef_e dv[w,e]) in element order).  The MFMA pass
// computes every score to within a bound `band` of that value (both share base[v]; the
// k-term dot differs by at most 2 gamma_{k+4} sum|terms|), so a row whose band around the
// MFMA maximum holds ONE vertex is decided; a row with several (real ties: degenerate
// scenarios whose optimal duals are all in V) is re-decided by cut_fixup_kernel, which
// evaluates the logged in-band candidates in the restatement's order -- the same pick as the
// C port, bit for bit, at any tie.
//   candidate log: while a lane scans its vertices it appends every vertex whose MFMA score
//   reaches the running band [M - tol(M) - band, ...]; the band's floor only rises with M, so
//   the log is a superset of the final band (a jump past the band restarts it).
//     p_w   = weight_w / total_weight
//     alpha = g.r + sum_{e RHS} S_e,   beta = -T' g - sum_{e T} S_e e_{col_e}
// with g = sum_v h_v pi_v,  h_v = sum_{w: a(w)=v} p_w,  S_e = sum_w p_w PK[a(w),e] dv[w,e].
// (Same value as the reference's per-scenario loop, re-associated.)
//
// Kernels, by file (cut_common.h: what the files share; cut_plan.h: the launch plan of a cut):
//  cut_prep.hip
//   cut_pk_kernel      PK (|V| x k4 row-major), PKT (k4 x vcap) and PKO (PK's columns in the
//                      restated element order) gathers of new vertices
//   cut_vbase_kernel   base[v] = pi_v . (r - T x) in index order (8|V|(m+1) bytes) and the
//                      decision band (max_v |base[v]| + sum_e |PK[v,e] coef_e| dmax_e)
//   cut_pktc_kernel    PKTc = coef(x) * PKT plus the base row: the chunk source of the argmax
//   cut_pkq_kernel     the integer pass's chunk source (fixed-point int8 limbs, cut_i8.h)
//  cut_argmax.hip
//   cut_argmax2_kernel MFMA score tiles (v_mfma_f64_16x16x4f64: 32 vertices x 32 scenarios
//                      per wave and chunk), vertex chunks DMA'd into LDS, running max/argmax
//                      per scenario in registers; per-wave partial sums; h via uint64
//                      fixed-point atomics (exact and order independent -> identical on any
//                      rank count); the last round's tiles split by vertex range
//   cut_argmax3_kernel the same pass with fp32 operands (v_mfma_f32_16x16x4f32), the base added in fp64
//   cut_argmax4_kernel the same pass with fixed-point int8-limb operands
//                      (v_mfma_i32_16x16x64_i8, cut_i8.h): exact integer sums, the default
//  cut_fixup.hip
//   cut_tail_merge_kernel  per-range results of the split tiles merged in vertex order
//   cut_fixup_kernel   scenarios with several vertices in the decision band: their logged
//                      candidates re-scored in the restatement's order and decided by its rule
//   cut_rescan_kernel  the few whose candidate log overflowed: every vertex re-scored
//  cut_kernel.hip (this file: the driver, cut_partial_impl, and the C entry points)
//   cut_reduce_kernel  deterministic fixed-order sum of the partial slots
//   cut_g_kernel(s)    g = sum_v h_v pi_v (two-level, fixed order)
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "cut_common.h"

namespace twosd {

// sums[c] = sum over slots of partial[slot][c], c < k+1, in a fixed order: block b sums
// the slot range [b*per, (b+1)*per) with a fixed-shape in-block tree, then the last level
// adds the block results in block order (deterministic, independent of timing).
constexpr int kReduceBlocks = 64;
__global__ void __launch_bounds__(256) cut_reduce1_kernel(int slots, int width, const double *__restrict__ partial,
                                                          double *__restrict__ part2) {
    __shared__ double sh[256];
    const int b = blockIdx.x, c = blockIdx.y;
    const int per = (slots + kReduceBlocks - 1) / kReduceBlocks;
    const int s0 = b * per, s1 = min(slots, s0 + per);
    double s = 0.0;
    for (int i = s0 + threadIdx.x; i < s1; i += 256) s += partial[(size_t)i * width + c];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part2[(size_t)c * kReduceBlocks + b] = sh[0];
}
__global__ void cut_reduce2_kernel(int width, const double *__restrict__ part2, double *__restrict__ sums) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= width) return;
    double s = 0.0;
    for (int b = 0; b < kReduceBlocks; ++b) s += part2[(size_t)c * kReduceBlocks + b];
    sums[c] = s;
}

// gpart[b][i] = sum_{v in chunk b} h_v * 2^-62 * V[v][i]
__global__ void cut_g_partial_kernel(int nv, int m, int chunk, const unsigned long long *__restrict__ hist,
                                     const double *__restrict__ V, double *__restrict__ gpart) {
    const int b = blockIdx.x;
    const int v0 = b * chunk, v1 = min(nv, v0 + chunk);
    for (int i = threadIdx.x; i < m; i += blockDim.x) {
        double s = 0.0;
        for (int v = v0; v < v1; ++v) {
            const unsigned long long h = hist[v];
            if (h) s = fma((double)h * (1.0 / kFix), V[(size_t)v * m + i], s);
        }
        gpart[(size_t)b * m + i] = s;
    }
}

__global__ void cut_g_final_kernel(int nb, int m, const double *__restrict__ gpart, double *__restrict__ gout) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += gpart[(size_t)b * m + i];
    gout[i] = s;
}

void cut_free(CutWs *w) { delete w; }

void cut_truncate_pk(twosd_ctx *c, int size) {
    // stored picks over vertices past `size` name vertices that no longer exist
    for (PickSet &h : c->reform.picks)
        if (h.live && h.nv > size) h.stale = true;
    if (c->last_cut_nv > size) c->last_cut_epi = -1;
    if (!c->cut_ws) return;
    CutWs *w = c->cut_ws.get();
    if (w->pk_count > size) w->pk_count = size;   // twin links point to lower vertices: still valid
}

void cut_invalidate_pk(twosd_ctx *c) {
    c->last_cut_epi = -1;
    if (!c->cut_ws) return;
    CutWs *w = c->cut_ws.get();
    w->pk_count = 0;
    w->rows.release();   // forces re-upload of the element rows (and their order)
}

// a cut that returns before the argmax (no scenarios) leaves no fixup counters: clear the last
// cut's, so twosd_cut_stats does not report them as this cut's
static int clear_cut_stats(twosd_ctx *c) {
    CutWs *w = c->cut_ws.get();
    if (w && w->fstats) {
        HIPCHK(hipMemsetAsync(w->fstats, 0, sizeof(unsigned long long) * CS_COUNT, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return TWOSD_OK;
}

// what one cut ran with (twosd_cut_debug_scores reads it back)
struct CutRun {
    CutShape sh;
    CutPlan pl;
    CutParams P;
};

// shape and plan of a cut over N scenarios, or the plan's refusal as the library's error
static int plan_cut(twosd_ctx *c, int N, const CutKnobs &kn, CutRun &run) {
    run.sh = CutShape{N, c->dvs.size, c->k, c->num_cus, cut_argmax_bpc(c->k, kn)};
    const CutPlan &pl = run.pl;
    switch (cut_plan(run.sh, kn, kCutKBs, kNumKB, run.pl)) {
    case CUT_PLAN_K_ENVELOPE:
        return fail(TWOSD_E_UNSUPPORTED, "k = %d random elements exceeds the cut kernel envelope (127)", c->k);
    case CUT_PLAN_LOG_SLOTS:
        return fail(TWOSD_E_UNSUPPORTED, "cut: %d scenarios need %zu candidate-log slots (32-bit offsets: at most %zu)", N,
                    std::max(pl.cand_need, pl.tcand_need), kn.log_max);
    case CUT_PLAN_OK: break;
    }
    return TWOSD_OK;
}

// host: bvec = r - (T x) as the reference writes it (`coef.rhs - coef.transfer * x`,
// subprob.jl:147): T x accumulated from zero column by column, as SparseArrays' CSC mat-vec
// does (tx[i] += T[i][j] * x[j] for j ascending, no contraction), then subtracted from r
// (oracle_build_cut, twosd_ref._seq_base); coef
void host_bvec_coef(const twosd_ctx *c, const double *x, int k4, std::vector<double> &bvec, std::vector<double> &coef) {
    const int m = c->L.m, n1 = c->n1, k = c->k;
    bvec.assign(m, 0.0);
    coef.assign(k4, 0.0);
    for (int i = 0; i < m; ++i) {
#pragma clang fp contract(off)
        double tx = 0.0;
        for (int jj = 0; jj < n1; ++jj) tx = tx + c->T[(size_t)i * n1 + jj] * x[jj];
        bvec[i] = c->r[i] - tx;
    }
    for (int e = 0; e < k; ++e) coef[e] = c->pos_col[e] < 0 ? 1.0 : -x[c->pos_col[e]];
}

// the per-x vectors of the cut's operands: coef_e(x), bvec = r - T x, and g
int cut_size_vectors(CutWs *w, int m) {
    int rc;
    if (!w->coef || !w->bvec || !w->g || w->vec_m != m) {
        if ((rc = w->coef.alloc(256)) || (rc = w->bvec.alloc(m)) || (rc = w->g.alloc(m))) return rc;
        w->vec_m = m;
    }
    return TWOSD_OK;
}

// every buffer of a cut but the epigraph's dmax (cut_fold_dmax), sized from its shape and plan
static int size_workspace(CutWs *w, const CutShape &sh, const CutPlan &pl, int m) {
    const size_t N = sh.N, nv = sh.nv, k = sh.k, tp = (size_t)pl.ntail * pl.S, vcap32 = pl.vcap32;
    int rc;
    if ((rc = cut_size_vectors(w, m))) return rc;
    if ((rc = w->base.fit(nv))) return rc;
    if ((rc = w->arg.fit(N)) || (rc = w->val.fit(N)) || (rc = w->flag.fit(N))) return rc;
    if ((rc = w->tp_m.fit(tp)) || (rc = w->tp_i.fit(tp)) || (rc = w->tp_f.fit(tp))) return rc;
    if ((rc = w->cand.fit(pl.cand_need)) || (rc = w->tcand.fit(pl.tcand_need))) return rc;
    if (!w->band_bits && (rc = w->band_bits.alloc(BAND_COUNT))) return rc;
    if (!w->fstats && (rc = w->fstats.alloc(CS_COUNT))) return rc;
    if ((rc = w->partial.fit(pl.slots * (k + 1))) || (rc = w->part2.fit((k + 1) * kReduceBlocks))) return rc;
    if (pl.hist_lds && (rc = w->hist_part.fit((size_t)pl.nblocks * nv))) return rc;
    if ((rc = w->PKTc.fit((size_t)pl.rows * vcap32)) || (rc = w->vmap.fit(nv))) return rc;
    if (!w->nvc && (rc = w->nvc.alloc(1))) return rc;
    if (nv * pl.k4 > w->PKOc.cap && ((rc = w->PKOc.alloc(nv * pl.k4)) || (rc = w->basec.alloc(vcap32)))) return rc;
    if (pl.want32 && ((rc = w->PKTc32.fit((size_t)pl.rows32 * vcap32)) || (rc = w->basec32.fit(vcap32)))) return rc;
    if (pl.wanti8) {
        if ((rc = w->PKq.fit((vcap32 / 32) * i8_chunk_bytes(pl.KS8))) || (rc = w->scq.fit(vcap32))) return rc;
        if (!w->dsc && (rc = w->dsc.alloc(128))) return rc;
    }
    return TWOSD_OK;
}

// the kernels' parameter block, every field, from the cut's shape and plan, the sized workspace and
// the epigraph; d_hist: where the vertex histogram goes
static CutParams cut_params(const CutShape &sh, const CutPlan &pl, const CutWs *w, const EpiDevice &E, double tie_rel,
                            double total_weight, unsigned long long *d_hist) {
    CutParams P{};
    P.N = sh.N; P.k = sh.k; P.k4 = pl.k4; P.nv = sh.nv; P.vcap = w->pk_vcap; P.m = w->m;
    P.hist_lds = pl.hist_lds;
    P.tie_rel = tie_rel; P.inv_total = 1.0 / total_weight;
    P.dv = E.d_dv; P.w = E.d_w; P.coef = w->coef;
    P.PK = w->PK; P.PKT = w->PKT; P.PKO = w->PKO;
    P.PKTc = w->PKTc; P.vcap32 = pl.vcap32;
    P.vmap = w->vmap; P.nvc = w->nvc; P.PKOc = w->PKOc; P.basec = w->basec; P.base = w->base; P.eord = w->eord;
    P.band_bits = w->band_bits + BAND_ACTIVE;
    P.mode = w->band_bits + BAND_PASS;
    P.basec32 = w->basec32; P.PKq = w->PKq; P.scq = w->scq; P.dsc = w->dsc; P.PKTc32 = w->PKTc32;
    P.band_scale = pl.band_scale;
    P.arg = w->arg; P.val = w->val; P.flag = w->flag;
    P.cand = w->cand; P.fstats = w->fstats; P.tcand = w->tcand;
    P.hist = d_hist; P.hist_part = w->hist_part; P.partial = w->partial;
    P.full_units = pl.full; P.tail_S = pl.S; P.fx_gs = pl.fx_gs;
    P.tp_m = w->tp_m; P.tp_i = w->tp_i; P.tp_f = w->tp_f;
    return P;
}

// argmax + partial sums over scenarios [0, N) of epigraph epi at x.  Fills d_hist (nv),
// d_sums (k+1), w->arg / w->val.  total_weight: global total scenario weight.
static int cut_partial_impl(twosd_ctx *c, int epi, const double *x, double tie_rel, double total_weight,
                            unsigned long long *d_hist, double *d_sums, CutRun &run) {
    CutWs *w = cws(c);
    const EpiDevice &E = c->epis[epi];
    const int N = E.count, k = c->k, m = c->L.m, nv = c->dvs.size;
    const CutKnobs kn = cut_knobs();
    int rc;
    if ((rc = update_pk(c))) return rc;
    if ((rc = plan_cut(c, N, kn, run))) return rc;
    const CutPlan &pl = run.pl;
    host_bvec_coef(c, x, pl.k4, w->h_bvec, w->h_coef);
    if ((rc = size_workspace(w, run.sh, pl, m))) return rc;
    HIPCHK(hipMemcpyAsync(w->coef, w->h_coef.data(), sizeof(double) * pl.k4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(w->bvec, w->h_bvec.data(), sizeof(double) * m, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(w->fstats, 0, sizeof(unsigned long long) * CS_COUNT, c->stream));
    if ((rc = cut_fold_dmax(c, epi, N, k))) return rc;
    HIPCHK(hipMemsetAsync(d_hist, 0, sizeof(unsigned long long) * std::max(nv, 1), c->stream));
    HIPCHK(hipMemsetAsync(w->band_bits, 0, sizeof(unsigned long long) * BAND_COUNT, c->stream));
    cut_operand_stage(c, epi, run.sh, pl, kn.twins);
    run.P = cut_params(run.sh, pl, w, E, tie_rel, total_weight, d_hist);
    cut_argmax_stage(pl, run.P, c->stream);
    cut_fixup_stage(pl, run.P, c->stream);
    hipLaunchKernelGGL(cut_reduce1_kernel, dim3(kReduceBlocks, k + 1), dim3(256), 0, c->stream, (int)pl.slots, k + 1,
                       w->partial, w->part2);
    hipLaunchKernelGGL(cut_reduce2_kernel, dim3((k + 1 + 63) / 64), dim3(64), 0, c->stream, k + 1, w->part2, d_sums);
    HIPCHK(hipGetLastError());
    return TWOSD_OK;
}

// g = sum_v h_v pi_v, then alpha / beta on the host
static int cut_finalize_impl(twosd_ctx *c, const double *x, const unsigned long long *d_hist, const double *d_sums,
                             double *alpha, double *beta) {
    CutWs *w = cws(c);
    const int nv = c->dvs.size, m = c->L.m, k = c->k, n1 = c->n1;
    (void)x;
    // vertex chunks of 32 or more, at most 512 of them (each block reads its chunk's rows of V once)
    const int chunk = std::max(32, (nv + 511) / 512);
    const int nb = std::max(1, (nv + chunk - 1) / chunk);
    int rc;
    if ((rc = w->gpart.fit((size_t)nb * m))) return rc;
    hipLaunchKernelGGL(cut_g_partial_kernel, dim3(nb), dim3(256), 0, c->stream, nv, m, chunk, d_hist, c->dvs.V, w->gpart);
    hipLaunchKernelGGL(cut_g_final_kernel, dim3((m + 255) / 256), dim3(256), 0, c->stream, nb, m, w->gpart, w->g);
    HIPCHK(hipGetLastError());
    std::vector<double> g(m), sums(k + 1);
    HIPCHK(hipMemcpyAsync(g.data(), w->g, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(sums.data(), d_sums, sizeof(double) * (k + 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    double a = 0.0;
    for (int i = 0; i < m; ++i) a += g[i] * c->r[i];
    for (int jj = 0; jj < n1; ++jj) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) s += c->T[(size_t)i * n1 + jj] * g[i];
        beta[jj] = -s;
    }
    for (int e = 0; e < k; ++e) {
        if (c->pos_col[e] < 0) a += sums[1 + e];
        else beta[c->pos_col[e]] -= sums[1 + e];
    }
    // general bounds: the picks' weights sum to 1, so the shift's objective constant enters once
    // (here, after any all-reduce of the partials)
    *alpha = c->has_bounds ? a + c->c0 : a;
    return TWOSD_OK;
}

const int *cut_last_arg(twosd_ctx *c) { return c->cut_ws ? c->cut_ws->arg.p : nullptr; }
const double *cut_last_val(twosd_ctx *c) { return c->cut_ws ? c->cut_ws->val.p : nullptr; }

int cut_last_usable(twosd_ctx *c, int epi, const char *who, const char *verb) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "%s: no template", who);
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "%s: epigraph %d does not exist", who, epi);
    if (c->last_cut_epi < 0)
        return fail(TWOSD_E_STATE, "%s: no cut to %s the picks of (none built, or the template, the positions or "
                    "the vertex set were reset since)", who, verb);
    if (c->last_cut_epi != epi)
        return fail(TWOSD_E_STATE, "%s: the last cut was built on epigraph %d, not %d", who, c->last_cut_epi, epi);
    if (c->last_cut_n <= 0 || !cut_last_arg(c) || !cut_last_val(c))   // picks and scores are sized together
        return fail(TWOSD_E_STATE, "%s: the last cut of epigraph %d took the empty-epigraph path (no picks)", who, epi);
    return TWOSD_OK;
}

int cut_pk_current(twosd_ctx *c, const double **PK, int *k4) {
    int rc = update_pk(c);
    if (rc) return rc;
    *PK = c->cut_ws->PK;
    *k4 = c->cut_ws->pk_k4;
    return TWOSD_OK;
}

}  // namespace twosd

using namespace twosd;

static int check_cut_args(twosd_ctx *c, int epi, const double *x) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "build_cut: no template");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "build_cut: epigraph %d does not exist", epi);
    if (c->n1 > 0 && !x) return fail(TWOSD_E_ARG, "build_cut: x is NULL");
    if (c->dvs.size == 0)
        return fail(TWOSD_E_STATE, "build_cut: the dual vertex set is empty (UndefRefError in build_sasa_cut, epigraph.jl:140)");
    return TWOSD_OK;
}

// ---- what twosd_build_cut and twosd_cut_partial / twosd_cut_finalize share
// device time between two completed events of the call into a timing slot
static void time_stage(twosd_ctx *c, EventSlot from, EventSlot to, TimeSlot slot) {
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[from], c->ev[to]);
    c->t_us[slot] = 1e3 * ms;
}

// the cut whose picks now sit in the workspace (n = 0: the empty-epigraph path)
static void set_last_cut(twosd_ctx *c, int epi, int n) {
    c->last_cut_epi = epi; c->last_cut_n = n; c->last_cut_nv = c->dvs.size;
}

// the cut's per-scenario maxima and picks to the host (each nullable)
static int copy_picks(twosd_ctx *c, int n, double *max_val, int *max_arg) {
    CutWs *w = cws(c);
    if (max_val) HIPCHK(hipMemcpy(max_val, w->val, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (max_val && c->has_bounds)   // scores of the canonical LP: the caller's objective adds the shift's constant
        for (int s = 0; s < n; ++s) max_val[s] += c->c0;
    if (max_arg) HIPCHK(hipMemcpy(max_arg, w->arg, sizeof(int) * n, hipMemcpyDeviceToHost));
    return TWOSD_OK;
}

extern "C" int twosd_build_cut(twosd_ctx *c, int epi, const double *x, double tie_rel, double *alpha, double *beta,
                               double *weight_mark, double *max_val, int *max_arg) {
    int rc = check_cut_args(c, epi, x);
    if (rc) return rc;
    if (!alpha || (c->n1 > 0 && !beta)) return fail(TWOSD_E_ARG, "build_cut: alpha/beta NULL");
    HIPCHK(hipSetDevice(c->device));
    const EpiDevice &E = c->epis[epi];
    CutWs *w = cws(c);
    if ((rc = w->hist.fit(c->dvs.size))) return rc;
    if ((rc = w->sums.fit(c->k + 1))) return rc;
    c->last_cut_epi = -1;   // set again once this cut's picks are in place (twosd_picks_keep)
    if (E.count == 0 || E.total_weight <= 0.0) {
        set_last_cut(c, epi, 0);
        // no scenarios: the reference returns the zero cut with weight_mark = total weight
        *alpha = 0.0;
        for (int j = 0; j < c->n1; ++j) beta[j] = 0.0;
        if (weight_mark) *weight_mark = E.total_weight;
        return clear_cut_stats(c);
    }
    CutRun run;
    HIPCHK(hipEventRecord(c->ev[EV_MARK_0], c->stream));
    if ((rc = cut_partial_impl(c, epi, x, tie_rel, E.total_weight, w->hist, w->sums, run))) return rc;
    HIPCHK(hipEventRecord(c->ev[EV_MARK_1], c->stream));
    if ((rc = cut_finalize_impl(c, x, w->hist, w->sums, alpha, beta))) return rc;
    HIPCHK(hipEventRecord(c->ev[EV_MARK_2], c->stream));
    HIPCHK(hipEventSynchronize(c->ev[EV_MARK_2]));
    time_stage(c, EV_MARK_0, EV_MARK_1, T_CUT_PARTIAL);
    time_stage(c, EV_MARK_1, EV_MARK_2, T_CUT_FINALIZE);
    set_last_cut(c, epi, E.count);
    if (weight_mark) *weight_mark = E.total_weight;
    return copy_picks(c, E.count, max_val, max_arg);
}

extern "C" int twosd_cut_stats(twosd_ctx *c, int64_t *out) {
    if (!c || !out) return fail(TWOSD_E_ARG, "cut_stats: NULL");
    for (int i = 0; i < 4; ++i) out[i] = 0;
    CutWs *w = c->cut_ws.get();
    if (!w || !w->fstats) return TWOSD_OK;
    unsigned long long h[CS_COUNT] = {};
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(h, w->fstats, sizeof(h), hipMemcpyDeviceToHost));
    out[0] = (int64_t)h[CS_FIX_ROWS];
    out[1] = (int64_t)h[CS_FIX_CANDS];
    out[2] = (int64_t)h[CS_FIX_RESCANS];
    out[3] = (int64_t)h[CS_TWINS];
    if (getenv("TWOSD_CUT3_COUNT_PRINT"))   // diagnostic build -DTWOSD_CUT3_COUNT only
        fprintf(stderr, "argmax3: chunk steps %llu, past the prefilter %llu, lanes past it %llu\n", h[CS_F32_STEPS], h[CS_F32_RARE],
                h[CS_F32_LANES]);
    if (getenv("TWOSD_FIX_STAMPS_PRINT")) {
        static const char *const phase[CS_FIX_STAMPS] = {"rows/setup", "deltas", "list", "chains", "decide", "sums"};
        fprintf(stderr, "fixup stamps (cycles summed over waves):");
        for (int i = 0; i < CS_FIX_STAMPS; ++i) fprintf(stderr, " %s %llu", phase[i], h[CS_FIX_STAMP0 + i]);
        fprintf(stderr, "\n");
    }
    return TWOSD_OK;
}

// the last cut's band_bits (zeros before the first cut), by BandSlot
static int read_band_bits(twosd_ctx *c, unsigned long long (&h)[BAND_COUNT]) {
    memset(h, 0, sizeof(h));
    CutWs *w = c->cut_ws.get();
    if (!w || !w->band_bits) return TWOSD_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(h, w->band_bits, sizeof(h), hipMemcpyDeviceToHost));
    return TWOSD_OK;
}

extern "C" int twosd_cut_pass(twosd_ctx *c, int *fp32, double *band) {
    if (!c || !fp32) return fail(TWOSD_E_ARG, "cut_pass: NULL");
    *fp32 = 0;
    if (band) *band = 0.0;
    unsigned long long h[BAND_COUNT];
    if (int rc = read_band_bits(c, h)) return rc;
    *fp32 = h[BAND_PASS] != 0;   // a reduced-precision pass ran: fp32 or integer (twosd_cut_pass_kind tells which)
    if (band) memcpy(band, &h[BAND_ACTIVE], sizeof(double));
    return TWOSD_OK;
}

extern "C" int twosd_cut_pass_kind(twosd_ctx *c, int *kind, int *limbs, int *pairs) {
    if (!c || !kind) return fail(TWOSD_E_ARG, "cut_pass_kind: NULL");
    *kind = 0;
    if (limbs) *limbs = ci8::kL;
    if (pairs) *pairs = ci8::kPairs;
    unsigned long long h[BAND_COUNT];
    if (int rc = read_band_bits(c, h)) return rc;
    *kind = (int)h[BAND_PASS];
    return TWOSD_OK;
}

extern "C" int twosd_cut_debug_scores(twosd_ctx *c, int epi, const double *x, float *out, int64_t cap, int *nvc_out,
                                      int *vmap_out) {
    int rc = check_cut_args(c, epi, x);
    if (rc) return rc;
    if (!out || !nvc_out) return fail(TWOSD_E_ARG, "cut_debug_scores: NULL");
    HIPCHK(hipSetDevice(c->device));
    const EpiDevice &E = c->epis[epi];
    CutWs *w = cws(c);
    const int nv = c->dvs.size, N = E.count;
    if (N <= 0 || !(E.total_weight > 0.0)) return fail(TWOSD_E_STATE, "cut_debug_scores: the epigraph has no scenarios");
    if ((long long)N * nv > (1ll << 20)) return fail(TWOSD_E_UNSUPPORTED, "cut_debug_scores: N |V| = %lld exceeds 2^20", (long long)N * nv);
    if ((rc = w->hist.fit(nv)) || (rc = w->sums.fit(c->k + 1))) return rc;
    // one cut at x prepares every operand of the pass (and runs whichever pass applies)
    c->last_cut_epi = -1;
    CutRun run;
    if ((rc = cut_partial_impl(c, epi, x, 0.0, E.total_weight, w->hist, w->sums, run))) return rc;
    if (!w->i8_ks) return fail(TWOSD_E_STATE, "cut_debug_scores: the integer pass is switched off (TWOSD_CUT_F32 / TWOSD_CUT_I8)");
    int nvc = 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(&nvc, w->nvc, sizeof(int), hipMemcpyDeviceToHost));
    if ((int64_t)N * nvc > cap) return fail(TWOSD_E_ARG, "cut_debug_scores: out holds %lld floats, %lld needed", (long long)cap, (long long)N * nvc);
    DevBuf<float, 4> d_out;
    if ((rc = d_out.alloc((size_t)N * nvc))) return rc;
    cut_scores_stage(run.pl, run.P, w->i8_ks, d_out.p, c->stream);   // the cut's own parameter block
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, d_out.p, sizeof(float) * (size_t)N * nvc, hipMemcpyDeviceToHost));
    if (vmap_out) HIPCHK(hipMemcpy(vmap_out, w->vmap, sizeof(int) * nvc, hipMemcpyDeviceToHost));
    *nvc_out = nvc;
    return TWOSD_OK;
}

extern "C" int twosd_cut_partial_len(twosd_ctx *c, int64_t *n_u64, int64_t *n_f64) {
    if (!c) return fail(TWOSD_E_ARG, "cut_partial_len: NULL");
    if (n_u64) *n_u64 = std::max(c->dvs.size, 1);
    if (n_f64) *n_f64 = c->k + 1;
    return TWOSD_OK;
}

extern "C" int twosd_cut_partial(twosd_ctx *c, int epi, const double *x, double tie_rel, double total_weight,
                                 uint64_t *d_hist, double *d_sums, double *max_val, int *max_arg) {
    int rc = check_cut_args(c, epi, x);
    if (rc) return rc;
    if (!d_hist || !d_sums) return fail(TWOSD_E_ARG, "cut_partial: device buffers NULL");
    if (!(total_weight > 0.0)) return fail(TWOSD_E_ARG, "cut_partial: total_weight must be > 0");
    HIPCHK(hipSetDevice(c->device));
    const EpiDevice &E = c->epis[epi];
    c->last_cut_epi = -1;
    if (E.count == 0) {
        set_last_cut(c, epi, 0);
        HIPCHK(hipMemsetAsync(d_hist, 0, sizeof(uint64_t) * std::max(c->dvs.size, 1), c->stream));
        HIPCHK(hipMemsetAsync(d_sums, 0, sizeof(double) * (c->k + 1), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return clear_cut_stats(c);
    }
    CutRun run;
    HIPCHK(hipEventRecord(c->ev[EV_MARK_0], c->stream));
    if ((rc = cut_partial_impl(c, epi, x, tie_rel, total_weight, (unsigned long long *)d_hist, d_sums, run))) return rc;
    HIPCHK(hipEventRecord(c->ev[EV_MARK_1], c->stream));
    HIPCHK(hipEventSynchronize(c->ev[EV_MARK_1]));
    time_stage(c, EV_MARK_0, EV_MARK_1, T_CUT_PARTIAL);
    set_last_cut(c, epi, E.count);
    return copy_picks(c, E.count, max_val, max_arg);
}

extern "C" int twosd_cut_finalize(twosd_ctx *c, const double *x, const uint64_t *d_hist, const double *d_sums,
                                  double *alpha, double *beta) {
    if (!c || !c->has_template || !d_hist || !d_sums || !alpha || (c->n1 > 0 && !beta))
        return fail(TWOSD_E_ARG, "cut_finalize: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord(c->ev[EV_MARK_1], c->stream));
    int rc = cut_finalize_impl(c, x, (const unsigned long long *)d_hist, d_sums, alpha, beta);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev[EV_MARK_2], c->stream));
    HIPCHK(hipEventSynchronize(c->ev[EV_MARK_2]));
    time_stage(c, EV_MARK_1, EV_MARK_2, T_CUT_FINALIZE);
    return TWOSD_OK;
}
