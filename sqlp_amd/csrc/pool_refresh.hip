// pool_refresh.hip -- the warm-start pool refresh at x: twosd_pool_refresh on one GPU, and the
// twosd_refresh_* family of the distributed refresh (one process per GPU).  Both run the same
// front end (refresh_front), bind the same source-table type (PgTable) and build the same pool
// bit for bit.  The pool itself (arrays, upload, validity) is basis_pool.hip's, the per-x preparation
// pool_select.hip's.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "twosd_internal.h"
#include "twosd_ctx.h"

using namespace twosd;

using Clock = std::chrono::steady_clock;
static double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// ---- pool refresh at x: the pool's bases are optimal near the x they were harvested at
// (storm: 8.9 pivots per scenario at the training x, 28-67 at SD candidates 25-37 % away), so a
// new x gets a pool of its own.  B^{-1} of a harvested basis is composed from its start basis
// and the eta file of its solve, B^{-1} = E_K..E_1 B_pb^{-1} (sparse row merges), so no
// refactorisation: the cost is the training solves plus O(K nnz) host work per basis.

// pi0 = c_B' B^{-1} from the composed rows, then the checks of host_basis.cpp; nullptr if the
// basis is usable
static const char *finish_composed(const twosd_ctx *c, PoolBasis &B) {
    const HostLP &L = c->L;
    pi0_from_rows(c, B);
    if (sparse_dual_infeasibility(L, B.head, B.pi0) > 1e-7) return "composed basis is not dual feasible";
    if (sparse_basis_residual(L, B.head, B.rptr, B.rcol, B.rval, 4) > 1e-8) return "composed B^{-1} inconsistent";
    return nullptr;
}

// Device build of the refreshed pool (pool_gpu.hip) from the eta files and heads of the
// training solves (rows = training scenarios in c->d_eo_* / c->d_head_out; the representatives
// in c->d_refresh_sel).  Two phases:
//   pg_compute   sources a = 0 (primary), a = 1..R (eta-file row d_refresh_sel[a - 1]) composed
//                column by column into an intermediate CSC and checked (d_pg_* arrays);
//   pg_assemble  the sources listed in `order` that passed the checks become pool[0..P), in
//                that order: the arrays upload_pool + prepare_elements would produce.
// The single-GPU refresh runs both on one source table; the distributed refresh
// (twosd_refresh_*) runs pg_compute on each rank's own representatives and pg_assemble on the
// table all ranks gathered.

// the two source tables of a context: what pg_compute fills, and what twosd_refresh_assemble
// gathers from the ranks' packs (the pointers are those of the buffers as they are now: bind
// again after a reserve)
static PgTable pg_local_table(twosd_ctx *c, int nsrc) {
    return PgTable{nsrc, c->d_pg_cnt, c->d_pg_tot, c->d_pg_valid, c->d_pg_ioff, c->d_pg_irow, c->d_pg_ival, nullptr};
}
static PgTable pg_gathered_table(twosd_ctx *c, int nsrc) {
    return PgTable{nsrc, c->d_gs_cnt, c->d_gs_tot, c->d_gs_valid, c->d_gs_ioff, c->d_gs_irow, c->d_gs_ival, c->d_gs_heads};
}

// workspace + PgArgs of a compute over nsrc sources (the template and start-pool fields; the
// caller binds the source table)
static int pg_args(twosd_ctx *c, int nsrc, PgArgs &A) {
    const HostLP &L = c->L;
    const int m = L.m;
    int rc;
    if ((rc = c->d_pg_pos.reserve((size_t)std::max(c->k, 1))) || (rc = c->d_pg_amax.reserve((size_t)nsrc)) ||
        (rc = c->d_pg_cnt.reserve(PgTable::cnt_size(nsrc, m))) || (rc = c->d_pg_tot.reserve(PgTable::tot_size(nsrc))) ||
        (rc = c->d_pg_valid.reserve((size_t)nsrc)) || (rc = c->d_pg_head0.reserve((size_t)m)) ||
        (rc = c->d_pg_d0p.reserve((size_t)64 * c->CH)) || (rc = c->d_pg_ioff.reserve((size_t)nsrc)))
        return rc;
    const PoolArrays pa = pool_arrays(c);   // the start pool
    HIPCHK(hipMemcpyAsync(c->d_pg_head0, c->bp.head0.data(), sizeof(int) * m, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_pg_d0p, pa.d0, sizeof(double) * 64 * c->CH, hipMemcpyDeviceToDevice, c->stream));
    if (c->k) HIPCHK(hipMemcpyAsync(c->d_pg_pos, c->pos_row.data(), sizeof(int) * c->k, hipMemcpyHostToDevice, c->stream));
    A = PgArgs{};
    A.m = m; A.n = L.n; A.MP = c->MP; A.CH = c->CH; A.R9 = c->R; A.k = c->k; A.kmax = c->eo_kmax;
    A.npool_old = (int)c->bp.bases.size();
    A.colptr = c->d_colptr; A.rowidx = c->d_rowidx; A.val = c->d_val; A.q = c->d_q; A.btype = c->d_btype;
    A.pos_row = c->d_pg_pos;
    A.bcp0 = pa.bcp; A.bci0 = pa.bci; A.bcv0 = pa.bcv;
    A.eo_pb = c->d_eo_pb; A.eo_K = c->d_eo_K; A.eo_off = c->d_eo_off; A.eo_etap = c->d_eo_etap;
    A.eo_etaoff = c->d_eo_etaoff; A.eo_eidx = c->d_eo_eidx; A.eo_evals = c->d_eo_evals;
    A.head0 = c->d_pg_head0; A.heads = c->d_head_out; A.src_row = c->d_refresh_sel;
    A.a0 = 0;
    A.amax = c->d_pg_amax;
    return TWOSD_OK;
}

// host copies of a source table (pinned staging): the per-source totals (4 each) and validity,
// the intermediate offsets (prefix of the nonzero counts) and their sum
struct PgHost {
    const int *tot = nullptr, *valid = nullptr;
    const long long *ioff = nullptr;
    long long inz = 0;
};

// compute phase over sources [0, nsrc) into the local table: FTRAN passes + counts and checks
static int pg_compute(twosd_ctx *c, int nsrc, PgArgs &A, PgHost &H, bool dbg) {
    int rc;
    if ((rc = pg_args(c, nsrc, A))) return rc;
    pg_bind(A, pg_local_table(c, nsrc));
    // the first pass keeps each source's nonzeros (up to sc_cap entries, sized from the last
    // build's largest source; at most 1.5 GiB in all) for pg_gather_kernel: one FTRAN per
    // column instead of two; a source past sc_cap runs the second FTRAN pass
    const int m = c->L.m;
    long long cap = c->pg_sc_cap > 0 ? c->pg_sc_cap : std::min<long long>((long long)m * m, 16384);
    if (getenv("TWOSD_PG_NOSCRATCH")) cap = 0;   // A/B knob: two FTRAN passes
    if (const char *e = getenv("TWOSD_PG_SCCAP")) cap = atoll(e);   // test hook: sources past it take pass 1
    cap = std::min(cap, ((3LL << 29) / 12) / std::max(nsrc, 1));
    if (cap > 0 && ((rc = c->d_pg_scrow.reserve((size_t)nsrc * cap)) || (rc = c->d_pg_scval.reserve((size_t)nsrc * cap)) ||
                    (rc = c->d_pg_scoff.reserve(PgTable::plane_size(nsrc, m)))))
        return rc;
    A.sc_cap = cap; A.sc_row = c->d_pg_scrow; A.sc_val = c->d_pg_scval; A.sc_off = c->d_pg_scoff;
    HIPCHK(pg_launch_ftran(A, 0, nsrc, c->stream));
    int *h_nz = c->stage[STG_PG_NZ].reserve<int>((size_t)nsrc);
    long long *h_ioff = c->stage[STG_PG_IOFF].reserve<long long>((size_t)nsrc);
    if (!h_nz || !h_ioff) return fail(TWOSD_E_DEVICE, "pool refresh: pinned staging allocation failed");
    HIPCHK(hipMemcpyAsync(h_nz, A.nztot, sizeof(int) * nsrc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    long long inz = 0, nzmax = 0;
    int over = 0;
    for (int a = 0; a < nsrc; ++a) {
        h_ioff[a] = inz;
        inz += h_nz[a];
        nzmax = std::max<long long>(nzmax, h_nz[a]);
        over += h_nz[a] > cap;
    }
    if ((rc = c->d_pg_irow.reserve((size_t)inz)) || (rc = c->d_pg_ival.reserve((size_t)inz))) return rc;
    HIPCHK(hipMemcpyAsync(c->d_pg_ioff, h_ioff, sizeof(long long) * nsrc, hipMemcpyHostToDevice, c->stream));
    pg_bind(A, pg_local_table(c, nsrc));   // the intermediate CSC as reserved just now
    if (cap > 0) HIPCHK(pg_launch_gather(A, nsrc, c->stream));
    if (over || cap == 0) HIPCHK(pg_launch_ftran(A, 1, nsrc, c->stream));
    c->pg_sc_cap = std::max<long long>(1024, nzmax + nzmax / 2);   // the next build's scratch
    HIPCHK(pg_launch_count(A, nsrc, c->stream));
    int *ht = c->stage[STG_PG_TOT].reserve<int>((size_t)5 * nsrc);
    if (!ht) return fail(TWOSD_E_DEVICE, "pool refresh: pinned staging allocation failed");
    HIPCHK(hipMemcpyAsync(ht, A.tot, sizeof(int) * 4 * nsrc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ht + (size_t)4 * nsrc, A.valid, sizeof(int) * nsrc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (dbg) fprintf(stderr, "pg_compute: %d sources, %lld intermediate entries, largest %lld, %d past the scratch of %lld\n", nsrc, inz,
                     nzmax, over, cap);
    H.tot = ht;
    H.valid = ht + (size_t)4 * nsrc;
    H.ioff = h_ioff;
    H.inz = inz;
    return TWOSD_OK;
}

// assemble phase: pool = the sources of `order` (order[0] = 0, the primary) that passed, in
// order; A describes the source table (compute output or the gathered table)
static int pg_assemble(twosd_ctx *c, PgArgs &A, const PgHost &H, const std::vector<int> &order, bool dbg) {
    int rc;
    if (order.empty() || order[0] != 0 || !H.valid[0]) return 1;   // the primary failed the device checks: host path
    std::vector<int> map, off;
    std::vector<int64_t> acc(4, 0);
    for (int a : order) {
        if (!H.valid[a]) continue;
        map.push_back(a);
        for (int f = 0; f < 4; ++f) {
            off.push_back((int)acc[f]);
            acc[f] += H.tot[(size_t)a * 4 + f];
        }
        if (acc[0] > INT32_MAX || acc[1] > INT32_MAX || acc[2] * 64 > INT32_MAX || acc[3] > INT32_MAX)
            return fail(TWOSD_E_UNSUPPORTED, "basis pool too large (> 2^31 entries)");
    }
    const int P = (int)map.size();
    const auto t0 = Clock::now();
    if ((rc = c->d_pg_map.reserve((size_t)P)) || (rc = c->d_pg_off.reserve((size_t)4 * P))) return rc;
    // From here the live pool arrays are grown in place (a grown array does not keep its
    // contents) and then overwritten: a failure past this point leaves the pool's bases describing
    // arrays that no longer hold them.  The context then drops its basis (pool_dropped), so every
    // later solve fails cleanly (TWOSD_E_STATE) until twosd_compute_basis / twosd_set_basis
    // installs one.
    auto broken = [c](int code) { return pool_dropped(c, code); };
    if (const char *inj = getenv("TWOSD_INJECT_FAIL"); inj && !strcmp(inj, "refresh_fill"))   // test hook
        return broken(fail(TWOSD_E_DEVICE, "pool refresh: injected failure after the pool-array reservation"));
    HIPCHK(hipMemcpyAsync(c->d_pg_map, map.data(), sizeof(int) * P, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_pg_off, off.data(), sizeof(int) * 4 * P, hipMemcpyHostToDevice, c->stream));
    const size_t nz = (size_t)acc[0], kz = (size_t)acc[1], ez = (size_t)acc[2] * 64;
    if ((rc = pool_reserve(c, P, nz, kz, ez)) || (rc = c->d_sel_ptr.reserve((size_t)P + 1)) ||
        (rc = reserve_selection(c, P, (int)acc[3])))
        return broken(rc);
    // (a grown array is reallocated: the start pool's CSC was read only by the FTRAN passes)
    PgFill F{};
    F.P = P; F.map = c->d_pg_map; F.off = c->d_pg_off; F.sel_total = (int)acc[3]; F.d0_primary = c->d_pg_d0p;
    const PoolArrays pa = pool_arrays(c);   // as reserved just now
    F.brptr = pa.brptr; F.brcol = pa.brcol; F.brval = pa.brval; F.bcp = pa.bcp; F.bci = pa.bci; F.bcv = pa.bcv;
    F.kp = pa.kp; F.ke = pa.ke; F.kraw = pa.kraw; F.kslot = pa.kslot; F.kix = pa.kix; F.kv = pa.kv;
    F.hb0 = pa.hb0; F.basic0 = pa.basic0; F.bnnz = pa.bnnz; F.d0 = pa.d0; F.sel_ptr = c->d_sel_ptr;
    F.P0 = 0;
    if (pg_launch_fill(A, F, P, c->stream) != hipSuccess) return broken(fail(TWOSD_E_DEVICE, "pool refresh: fill launch failed"));
    // the pool's heads (hb0 = 4 head + type) stay on the device; a host head is fetched on first
    // use (pool_head)
    const auto t1 = Clock::now();
    pool_installed_from_device(c, P);
    if (dbg) fprintf(stderr, "pg_assemble: P=%d fill + heads %.2f ms, host pool %.2f ms\n", P, ms_between(t0, t1), ms_between(t1, Clock::now()));
    return TWOSD_OK;
}

// Returns 1, with the pool unchanged, when the LDS layouts do not fit or the primary fails the
// device checks (the caller then composes on the host).
static int refresh_build_device(twosd_ctx *c, int R, bool dbg) {
    if (!pg_supported(c->L.m, c->L.n, c->eo_kmax)) return 1;
    PgArgs A;
    PgHost H;
    int rc;
    if ((rc = pg_compute(c, R + 1, A, H, dbg))) return rc;
    std::vector<int> order(R + 1);
    for (int a = 0; a <= R; ++a) order[a] = a;
    return pg_assemble(c, A, H, order, dbg);
}

// pivot cap of the training solves of a refresh.  One wavefront solves one scenario, so a
// training launch lasts as long as its slowest scenario; the scenarios far from the current
// pool (tens of pivots) mostly end at rare bases.  Auto: 3 x the mean pivots of the last large
// batch, at least 32 (storm: 32-33; ssn, ~33 pivots a solve: ~100); none before any batch.
// Storm 1M, 4096-basis pool (profiles/r03/train_kcap_1M.txt): cap 32 vs none -- refresh
// 18.3 vs 25.6 ms, and the next solve 86.6 vs 108.5 ms (fewer pivots from the capped pool).
// The one statement of the rule (twosd_training_cap exposes it to the distributed refresh, which
// applies it to the all-reduced pivot sum and size of every rank): setting = TWOSD_TRAIN_KCAP if
// set, else the context's (twosd_set_refresh_kcap); > 0 that cap, < 0 none, 0 auto =
// max(32, ceil(3 sum / n)) in integers, none before any large batch.
static int training_cap_rule(const twosd_ctx *c, int64_t sum, int64_t n) {
    const char *e = getenv("TWOSD_TRAIN_KCAP");   // A/B knob
    const int setting = e ? atoi(e) : (c ? c->train_kcap : 0);
    if (setting > 0) return setting;
    if (setting < 0 || n <= 0 || sum <= 0) return 0;
    const int64_t q = (3 * sum + n - 1) / n;
    return (int)std::max<int64_t>(32, std::min<int64_t>(q, INT32_MAX));
}
static int train_kcap(const twosd_ctx *c) { return training_cap_rule(c, c->piv_ref_sum, c->piv_ref_n); }

extern "C" int twosd_training_cap(twosd_ctx *c, int64_t pivots_sum, int64_t scenarios, int *cap) {
    if (!cap) return fail(TWOSD_E_ARG, "training_cap: NULL");   // ctx NULL: setting 0 (host code only)
    if (pivots_sum < 0 || scenarios < 0) return fail(TWOSD_E_ARG, "training_cap: negative pivot sum / size");
    *cap = training_cap_rule(c, pivots_sum, scenarios);
    return TWOSD_OK;
}

extern "C" int twosd_refresh_cap_stats(twosd_ctx *c, int64_t *pivots_sum, int64_t *scenarios) {
    if (!c) return fail(TWOSD_E_ARG, "refresh_cap_stats: NULL");
    if (pivots_sum) *pivots_sum = c->piv_ref_sum;
    if (scenarios) *scenarios = c->piv_ref_n;
    return TWOSD_OK;
}

extern "C" int twosd_set_refresh_kcap(twosd_ctx *c, int kcap) {
    if (!c) return fail(TWOSD_E_ARG, "set_refresh_kcap: NULL");
    c->train_kcap = kcap;
    return TWOSD_OK;
}

// The training solves of a refresh (basis keys, eta files, final heads) under the pivot cap.  The
// auto cap follows the last batch's pivots at the previous x; when x moved far from the pool's x
// (bench with warmup 4: the x_EV pool trained from the primary basis, next x SD candidate 4 --
// 58.5 pivots a scenario against a cap of 35), most training scenarios hit the cap and the
// refresh would find almost no optimal bases.  If fewer than half end optimal, the training is
// solved again without a cap (one extra launch, only on such a jump).
static int refresh_training(twosd_ctx *c, const double *x, const double *d_dv, int count, int kcap, bool retry, int *n_opt, bool dbg) {
    LpRun o;
    o.want_bkey = true;
    o.want_etas = true;
    o.want_head = true;
    // training scenarios beyond the pivot cap only drop out of the basis count (one launch
    // lasts as long as its slowest scenario: with one scenario per wave the cap bounds it)
    o.kcap = kcap;
    int rc;
    if ((rc = run_lp(c, x, d_dv, count, o))) return rc;
    int opt = count;
    if (o.kcap > 0) {
        std::vector<int> st(count);
        HIPCHK(hipMemcpy(st.data(), c->d_status, sizeof(int) * count, hipMemcpyDeviceToHost));
        opt = (int)std::count(st.begin(), st.end(), (int)TWOSD_LP_OPTIMAL);
        if (retry && 2 * opt < count) {
            if (dbg) fprintf(stderr, "refresh training: %d of %d optimal under cap %d, solved again uncapped\n", opt, count, o.kcap);
            o.kcap = 0;
            if ((rc = run_lp(c, x, d_dv, count, o))) return rc;
        }
    }
    // The eta files share one arena, claimed through an atomic counter that keeps counting past
    // its end.  Files that did not fit are lost (K = -1), and which ones those are depends on the
    // order the waves finish in: solve again with an arena of the size this run asked for, so that
    // the refreshed pool does not depend on that order.  Past 2^31 entries (32-bit offsets) the
    // losses stay.
    HIPCHK(hipStreamSynchronize(c->stream));
    unsigned long long used64 = 0;
    HIPCHK(hipMemcpy(&used64, c->d_eo_used, sizeof(used64), hipMemcpyDeviceToHost));
    if (used64 > c->eo_cap && used64 <= (unsigned long long)INT32_MAX) {
        if (dbg) fprintf(stderr, "refresh training: eta files of %llu entries past the arena of %zu, solved again\n", used64, c->eo_cap);
        c->eo_min_cap = (size_t)std::min<unsigned long long>(used64 + used64 / 8, INT32_MAX);
        if ((rc = run_lp(c, x, d_dv, count, o))) return rc;
    }
    c->last_train_opt = opt;
    if (n_opt) *n_opt = opt;
    return TWOSD_OK;
}

// The front end of a refresh, shared by twosd_pool_refresh and twosd_refresh_train*: the argument
// checks (`who` prefixes the messages; args_ok is the entry point's own condition), the training
// solves at x from the current pool, and the distinct optimal bases read back: the training
// scenario each first occurs at (reps) and how often it occurs (cnts), in order of first
// occurrence.  kcap < 0: the context's own cap (train_kcap).  *untrained (nullable) is cleared
// once the arguments are accepted: the training overwrites what an earlier one left.
namespace {
struct RefreshFront {
    const EpiDevice *E = nullptr;
    const double *d_dv = nullptr;                 // the training deltas (count x k)
    std::vector<int> reps, cnts;
    Clock::time_point t0, t_trained, t_bases;     // start, after the training, after the read-back
};
}  // namespace
static int refresh_front(twosd_ctx *c, const char *who, int epi, const double *x, int first, int count, bool args_ok, int kcap,
                         bool retry, int *n_opt, bool *untrained, bool dbg, RefreshFront &F) {
    if (!c || !c->bp.has_basis) return fail(TWOSD_E_STATE, "%s: no primary basis", who);
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "%s: epigraph %d does not exist", who, epi);
    const EpiDevice &E = c->epis[epi];
    if (first < 0 || count < 1 || first + count > E.count || !args_ok || (c->n1 > 0 && !x)) return fail(TWOSD_E_ARG, "%s: bad arguments", who);
    if (c->CH <= 0) return fail(TWOSD_E_UNSUPPORTED, "%s: needs the hypersparse LP kernel", who);
    HIPCHK(hipSetDevice(c->device));
    F.t0 = Clock::now();
    F.E = &E;
    F.d_dv = E.d_dv + (size_t)first * c->k;
    if (untrained) *untrained = false;
    if (kcap < 0) kcap = train_kcap(c);
    int rc;
    // 1. training solves at x from the current pool: basis keys, eta files and heads by scenario
    if ((rc = refresh_training(c, x, F.d_dv, count, kcap, retry, n_opt, dbg))) return rc;
    if (dbg) {
        std::vector<int> st(count), itv(count);
        HIPCHK(hipMemcpy(st.data(), c->d_status, sizeof(int) * count, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(itv.data(), c->d_iters, sizeof(int) * count, hipMemcpyDeviceToHost));
        int h[8] = {0};
        long long itsum = 0;
        for (int s2 = 0; s2 < count; ++s2) { h[std::min(std::max(st[s2], 0), 7)]++; itsum += itv[s2]; }
        const double piv_mean_ref = c->piv_ref_n ? (double)c->piv_ref_sum / (double)c->piv_ref_n : 0.0;
        fprintf(stderr, "%s training: kcap %d (ref %.2f), pool %zu, statuses 0:%d 1:%d 2:%d 3:%d 4:%d 5+:%d, mean iters %.2f\n", who,
                kcap, piv_mean_ref, c->bp.bases.size(), h[0], h[1], h[2], h[3], h[4], h[5] + h[6] + h[7], (double)itsum / count);
    }
    F.t_trained = Clock::now();
    // 2. distinct optimal bases in order of first occurrence, with their counts
    const int *d_list = nullptr, *d_counts = nullptr;
    int U = 0;
    if ((rc = vkey_first_occurrences(c, count, c->d_bkey, c->d_status, &d_list, &U, &d_counts))) return rc;
    F.reps.resize(U);
    F.cnts.resize(U);
    if (U > 0) {
        HIPCHK(hipMemcpy(F.reps.data(), d_list, sizeof(int) * U, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(F.cnts.data(), d_counts, sizeof(int) * U, hipMemcpyDeviceToHost));
    }
    F.t_bases = Clock::now();
    return TWOSD_OK;
}

extern "C" int twosd_pool_refresh(twosd_ctx *c, int epi, const double *x, int first, int count, int max_pool,
                                  int *pool_size) {
    const bool dbg = getenv("TWOSD_DEBUG") != nullptr;
    RefreshFront F;
    int rc;
    if ((rc = refresh_front(c, "pool_refresh", epi, x, first, count, max_pool >= 1, -1, true, nullptr, nullptr, dbg, F))) return rc;
    const int m = c->L.m, U = (int)F.reps.size();
    // the most frequent bases first (ties: first occurrence), primary excluded
    std::vector<int> ord(U);
    for (int a = 0; a < U; ++a) ord[a] = a;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return F.cnts[a] > F.cnts[b]; });
    const int R = std::min(U, max_pool - 1);
    std::vector<int> sel(R);
    for (int a = 0; a < R; ++a) sel[a] = F.reps[ord[a]];
    std::vector<PoolBasis> fresh;
    bool device_built = false;
    c->last_refresh_ms[1] = ms_between(F.t_trained, F.t_bases);
    c->last_refresh_ms[2] = c->last_refresh_ms[3] = 0.0;
    if (R > 0 && !getenv("TWOSD_REFRESH_HOST")) {
        // 3. B^{-1} of the representatives from their eta files, and the pool arrays, on the device
        if ((rc = c->d_refresh_sel.fit((size_t)R))) return rc;
        HIPCHK(hipMemcpyAsync(c->d_refresh_sel, sel.data(), sizeof(int) * R, hipMemcpyHostToDevice, c->stream));
        const int dev = refresh_build_device(c, R, dbg);
        if (dev < 0) return dev;
        device_built = dev == 0;
        c->last_refresh_ms[2] = ms_between(F.t_bases, Clock::now());
    }
    if (R > 0 && !device_built) {
        // 3'. host path: compose on the host threads, then upload_pool + prepare_elements
        if ((rc = pool_host_rows(c))) return rc;   // start bases in host form
        const int kmax = c->eo_kmax;
        std::vector<int> pb(count), K(count), off(count), etap((size_t)count * kmax), etaoff((size_t)count * (kmax + 1)),
            heads((size_t)count * m);
        int used = 0;
        HIPCHK(hipMemcpy(pb.data(), c->d_eo_pb, sizeof(int) * count, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(K.data(), c->d_eo_K, sizeof(int) * count, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(off.data(), c->d_eo_off, sizeof(int) * count, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(etap.data(), c->d_eo_etap, sizeof(int) * etap.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(etaoff.data(), c->d_eo_etaoff, sizeof(int) * etaoff.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(heads.data(), c->d_head_out, sizeof(int) * heads.size(), hipMemcpyDeviceToHost));
        unsigned long long used64 = 0;
        HIPCHK(hipMemcpy(&used64, c->d_eo_used, sizeof(used64), hipMemcpyDeviceToHost));
        used = (int)std::min<unsigned long long>(used64, std::min<size_t>(c->eo_cap, INT32_MAX));
        std::vector<int> ei(std::max(used, 1));
        std::vector<double> ev(std::max(used, 1));
        if (used > 0) {
            HIPCHK(hipMemcpy(ei.data(), c->d_eo_eidx, sizeof(int) * used, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(ev.data(), c->d_eo_evals, sizeof(double) * used, hipMemcpyDeviceToHost));
        }
        const auto t2 = Clock::now();
        fresh.resize(R);
        std::vector<char> ok(R, 0);
        parallel_for(R, [&](int a) {   // threaded at any R: a compose is milliseconds of work
            const int l = sel[a];   // eta-file row: the training scenario
            if (K[l] < 0 || pb[l] < 0 || pb[l] >= (int)c->bp.bases.size()) return;
            PoolBasis &B = fresh[a];
            B.head.assign(heads.begin() + (size_t)l * m, heads.begin() + (size_t)(l + 1) * m);
            const int *eo = etaoff.data() + (size_t)l * (kmax + 1);
            const PoolBasis &B0 = c->bp.bases[pb[l]];
            compose_binv(m, B0.rptr, B0.rcol, B0.rval, K[l], etap.data() + (size_t)l * kmax, eo, ei.data() + off[l],
                         ev.data() + off[l], B.rptr, B.rcol, B.rval);
            ok[a] = finish_composed(c, B) == nullptr;
        }, 1);
        c->last_refresh_ms[2] = ms_between(t2, Clock::now());
        pool_replace_host_bases(c, fresh, ok);
    }
    // R == 0 (no training scenario optimal): the current pool stays (any pool basis is a valid
    // start; dropping to the primary basis alone would cost ~90 pivots a scenario)
    const auto tb = Clock::now();
    // training box of the deltas (selection row pruning), as twosd_pool_build; cached per
    // training range
    if ((rc = training_box(c, *F.E, epi, first, count, c->sel_lo, c->sel_hi, &c->sel_box))) return rc;
    const auto tu = Clock::now();
    const bool host_built = R > 0 && !device_built;   // R == 0: the pool is unchanged
    if (host_built && (rc = upload_pool(c))) return rc;
    const auto tua = Clock::now();
    if (host_built && (rc = prepare_elements(c))) return rc;
    const auto t3 = Clock::now();
    if (dbg)
        fprintf(stderr, "pool_refresh: train %.2f, keys %.2f, build %.2f, box %.2f, upload_pool %.2f, elements %.2f ms (R=%d)\n",
                ms_between(F.t0, F.t_trained), ms_between(F.t_trained, F.t_bases), ms_between(F.t_bases, tb), ms_between(tb, tu),
                ms_between(tu, tua), ms_between(tua, t3), R);
    c->last_refresh_ms[0] = ms_between(F.t0, F.t_trained);
    c->last_refresh_ms[3] = ms_between(tu, t3);
    c->last_refresh_ms[4] = ms_between(F.t0, t3);
    if (pool_size) *pool_size = (int)c->bp.bases.size();
    return TWOSD_OK;
}

// ---- distributed pool refresh -------------------------------------------------------------
// The refresh of twosd_pool_refresh split over the ranks (one process per GPU, the pool
// replicated): each rank solves its slice of the training scenarios (twosd_refresh_train), the
// ranks exchange the distinct optimal bases with their counts and pick the same most frequent
// max_pool - 1 (the caller's selection, sqlp_amd/dist.py), each rank composes the B^{-1} of the
// picked bases whose first occurrence it holds (twosd_refresh_build_local -> a pack of the
// intermediate CSC, counts and heads), the packs are all-gathered, and every rank assembles the
// same pool from the gathered table (twosd_refresh_assemble).  With the training scenarios
// split contiguously the pool equals the single-rank refresh of all of them, bit for bit.

// pack: 8-byte aligned sections of n sources with nz intermediate entries.  The byte layout is
// part of the exchange between ranks, which may run different builds of the library: it must not
// change (rt_sections below names what each section holds, not where it lies).
struct RtPack {
    size_t heads, cnt, tot, nztot, valid, irow, ival, bytes;
};
static inline size_t al8(size_t b) { return (b + 7) & ~(size_t)7; }
static RtPack rt_layout(long long n, long long nz, int m) {
    RtPack L{};
    size_t o = 32;   // header: n, nz, bytes, m (int64)
    L.heads = o; o = al8(o + sizeof(int) * (size_t)n * m);
    L.cnt = o; o = al8(o + sizeof(int) * 4 * (size_t)n * m);
    L.tot = o; o = al8(o + sizeof(int) * 4 * (size_t)n);
    L.nztot = o; o = al8(o + sizeof(int) * (size_t)n);
    L.valid = o; o = al8(o + sizeof(int) * (size_t)n);
    L.irow = o; o = al8(o + sizeof(int) * (size_t)nz);
    L.ival = o; o = al8(o + sizeof(double) * (size_t)nz);
    L.bytes = o;
    return L;
}

// The sections of a pack L of n sources with nz intermediate entries, against sources [a, a + n)
// of table T whose entries start at z: f(table address, pack offset, bytes) for the heads (a
// gathered table only; a >= 1), the four cnt planes, tot, nztot, valid, irow and ival.  The one
// list behind both directions: table -> pack (twosd_refresh_build_local) and pack -> table
// (twosd_refresh_assemble).
template <typename F>
static void rt_sections(const PgTable &T, int m, long long a, long long n, long long z, long long nz, const RtPack &L, F f) {
    const size_t nm = (size_t)n * m;
    if (T.gheads) f(T.gheads + (size_t)(a - 1) * m, L.heads, sizeof(int) * nm);
    for (int p = 0; p < 4; ++p) f(T.plane(p, m) + (size_t)a * m, L.cnt + sizeof(int) * p * nm, sizeof(int) * nm);
    f(T.tot + 4 * a, L.tot, sizeof(int) * 4 * n);
    f(T.nztot() + a, L.nztot, sizeof(int) * n);
    f(T.valid + a, L.valid, sizeof(int) * n);
    f(T.irow + z, L.irow, sizeof(int) * nz);
    f(T.ival + z, L.ival, sizeof(double) * nz);
}

// rows src_row[j] of the training heads -> out row j
__global__ void rt_heads_kernel(int n, int m, const int *__restrict__ heads, const int *__restrict__ src_row, int *__restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n * m; i += (size_t)gridDim.x * blockDim.x)
        out[i] = heads[(size_t)src_row[i / m] * m + i % m];
}

// batched copy: segment blockIdx.y = (src, dst, 4-byte words)
struct CopySeg { const int *src; int *dst; long long words; };
__global__ void rt_copy_kernel(const CopySeg *__restrict__ seg) {
    const CopySeg S = seg[blockIdx.y];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < S.words; i += (long long)gridDim.x * blockDim.x)
        S.dst[i] = S.src[i];
}
static void add_seg(std::vector<CopySeg> &seg, const void *src, void *dst, size_t bytes) {
    if (bytes) seg.push_back({static_cast<const int *>(src), static_cast<int *>(dst), (long long)(bytes / 4)});
}
static int rt_copy(twosd_ctx *c, const std::vector<CopySeg> &segs) {
    if (segs.empty()) return TWOSD_OK;
    CopySeg *h = c->stage[STG_RT_SEG].reserve<CopySeg>(segs.size());
    if (!h) return fail(TWOSD_E_DEVICE, "refresh: pinned staging allocation failed");
    std::copy(segs.begin(), segs.end(), h);
    if (int rc = c->d_gs_seg.fit(sizeof(CopySeg) * std::max<size_t>(segs.size(), 64))) return rc;
    HIPCHK(hipMemcpyAsync(c->d_gs_seg, h, sizeof(CopySeg) * segs.size(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(rt_copy_kernel, dim3(64, (unsigned)segs.size()), dim3(256), 0, c->stream, (const CopySeg *)c->d_gs_seg.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));   // the staging buffer is reused by the next call
    return TWOSD_OK;
}

// kcap: the training pivot cap (> 0; 0 none; < 0 the context's own); retry: solve again uncapped
// when fewer than half end optimal (the single-rank rule, decided by this rank alone)
static int refresh_train_impl(twosd_ctx *c, int epi, const double *x, int first, int count, int kcap, bool retry,
                              int *n_bases, int *n_opt, double *box_lo, double *box_hi) {
    const bool dbg = getenv("TWOSD_DEBUG") != nullptr;
    RefreshFront F;
    int rc;
    if ((rc = refresh_front(c, "refresh_train", epi, x, first, count, n_bases != nullptr, kcap, retry, n_opt,
                            c ? &c->rt_trained : nullptr, dbg, F)))
        return rc;
    const int U = (int)F.reps.size();
    c->rt_reps.swap(F.reps);
    c->rt_counts.swap(F.cnts);
    c->rt_keys.resize(U);
    if (U > 0) {
        std::vector<unsigned long long> bk(count);
        HIPCHK(hipMemcpy(bk.data(), c->d_bkey, sizeof(unsigned long long) * count, hipMemcpyDeviceToHost));
        for (int a = 0; a < U; ++a) c->rt_keys[a] = bk[c->rt_reps[a]];
    }
    // training box of the slice (cached per training range, as the single-rank refresh); the
    // range is also the slice twosd_refresh_build_local checks its representatives against
    if ((rc = training_box(c, *F.E, epi, first, count, c->rt_lo, c->rt_hi, &c->rt_box))) return rc;
    c->rt_box = BoxCache{epi, first, count, F.E->count};
    if (box_lo) std::copy(c->rt_lo.begin(), c->rt_lo.end(), box_lo);
    if (box_hi) std::copy(c->rt_hi.begin(), c->rt_hi.end(), box_hi);
    c->rt_nown = -1;
    c->rt_trained = true;
    c->last_refresh_ms[0] = ms_between(F.t0, F.t_trained);
    c->last_refresh_ms[1] = ms_between(F.t_trained, Clock::now());
    *n_bases = U;
    return TWOSD_OK;
}

extern "C" int twosd_refresh_train(twosd_ctx *c, int epi, const double *x, int first, int count, int *n_bases,
                                   double *box_lo, double *box_hi) {
    if (!c) return fail(TWOSD_E_ARG, "refresh_train: NULL context");
    return refresh_train_impl(c, epi, x, first, count, -1, true, n_bases, nullptr, box_lo, box_hi);
}

extern "C" int twosd_refresh_train_ex(twosd_ctx *c, int epi, const double *x, int first, int count, int kcap, int *n_bases,
                                      int *n_optimal, double *box_lo, double *box_hi) {
    return refresh_train_impl(c, epi, x, first, count, kcap > 0 ? kcap : 0, false, n_bases, n_optimal, box_lo, box_hi);
}

extern "C" int twosd_refresh_train_bases(twosd_ctx *c, uint64_t *keys, int *counts, int *reps) {
    if (!c || !c->rt_trained) return fail(TWOSD_E_STATE, "refresh_train_bases: no training solve (twosd_refresh_train)");
    const size_t U = c->rt_keys.size();
    if (keys) std::copy(c->rt_keys.begin(), c->rt_keys.end(), keys);
    if (counts) std::copy(c->rt_counts.begin(), c->rt_counts.end(), counts);
    if (reps) std::copy(c->rt_reps.begin(), c->rt_reps.begin() + U, reps);
    return TWOSD_OK;
}

extern "C" int twosd_refresh_build_local(twosd_ctx *c, int n_own, const int *reps, int64_t *pack_bytes) {
    if (!c || !c->rt_trained) return fail(TWOSD_E_STATE, "refresh_build_local: no training solve (twosd_refresh_train)");
    if (n_own < 0 || (n_own > 0 && !reps) || !pack_bytes) return fail(TWOSD_E_ARG, "refresh_build_local: bad arguments");
    for (int j = 0; j < n_own; ++j)
        if (reps[j] < 0 || reps[j] >= c->rt_box.count) return fail(TWOSD_E_ARG, "refresh_build_local: representative %d outside the slice", reps[j]);
    if (!pg_supported(c->L.m, c->L.n, c->eo_kmax))
        return fail(TWOSD_E_UNSUPPORTED, "refresh_build_local: the device pool build does not fit this template");
    HIPCHK(hipSetDevice(c->device));
    const auto t0 = Clock::now();
    const int m = c->L.m;
    int rc;
    if ((rc = c->d_refresh_sel.fit((size_t)std::max(n_own, 1)))) return rc;
    if (n_own) HIPCHK(hipMemcpyAsync(c->d_refresh_sel, reps, sizeof(int) * n_own, hipMemcpyHostToDevice, c->stream));
    PgArgs A;
    PgHost H;
    const int nsrc = n_own + 1;
    if ((rc = pg_compute(c, nsrc, A, H, getenv("TWOSD_DEBUG") != nullptr))) return rc;
    // the pack holds sources 1..n_own; the primary's nz0 entries stay local (every rank has them)
    const long long nz0 = n_own ? H.ioff[1] : H.inz, nz = H.inz - nz0;
    const RtPack L = rt_layout(n_own, nz, m);
    if ((rc = c->d_rt_pack.reserve(L.bytes))) return rc;
    long long *hdr = c->stage[STG_RT_HDR].reserve<long long>(4);
    if (!hdr) return fail(TWOSD_E_DEVICE, "refresh: pinned staging allocation failed");
    hdr[0] = n_own; hdr[1] = nz; hdr[2] = (long long)L.bytes; hdr[3] = m;
    HIPCHK(hipMemcpyAsync(c->d_rt_pack, hdr, 32, hipMemcpyHostToDevice, c->stream));
    char *P = c->d_rt_pack;
    if (n_own) {
        hipLaunchKernelGGL(rt_heads_kernel, dim3(std::min(1024, (n_own * m + 255) / 256)), dim3(256), 0, c->stream, n_own, m,
                           c->d_head_out, c->d_refresh_sel, reinterpret_cast<int *>(P + L.heads));
        HIPCHK(hipGetLastError());
    }
    std::vector<CopySeg> seg;   // the heads came from rt_heads_kernel: the local table has none
    rt_sections(pg_local_table(c, nsrc), m, 1, n_own, nz0, nz, L,
                [&](const void *t, size_t at, size_t bytes) { add_seg(seg, t, P + at, bytes); });
    if ((rc = rt_copy(c, seg))) return rc;
    c->rt_nz0 = nz0;
    c->rt_nsrc_local = nsrc;
    c->rt_nown = n_own;
    c->last_refresh_ms[2] = ms_between(t0, Clock::now());
    *pack_bytes = (int64_t)L.bytes;
    return TWOSD_OK;
}

extern "C" int twosd_refresh_pack(twosd_ctx *c, void *d_dst) {
    if (!c || c->rt_nown < 0 || !d_dst) return fail(TWOSD_E_STATE, "refresh_pack: no local build (twosd_refresh_build_local)");
    HIPCHK(hipSetDevice(c->device));
    long long bytes = 0;
    HIPCHK(hipMemcpy(&bytes, c->d_rt_pack + 16, sizeof(bytes), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpyAsync(d_dst, c->d_rt_pack, (size_t)bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return TWOSD_OK;
}

extern "C" int twosd_refresh_assemble(twosd_ctx *c, int G, const void *d_packs, int64_t stride, int R, const int *order,
                                      const double *box_lo, const double *box_hi, int *pool_size) {
    if (!c || c->rt_nown < 0) return fail(TWOSD_E_STATE, "refresh_assemble: no local build (twosd_refresh_build_local)");
    if (G < 1 || !d_packs || stride < 32 || (stride & 7) || R < 0 || (R > 0 && !order) || (c->k > 0 && (!box_lo || !box_hi)))
        return fail(TWOSD_E_ARG, "refresh_assemble: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    const bool dbg = getenv("TWOSD_DEBUG") != nullptr;
    const auto t0 = Clock::now();
    const int m = c->L.m;
    int rc;
    const char *packs = static_cast<const char *>(d_packs);
    std::vector<long long> hdr((size_t)4 * G);
    HIPCHK(hipMemcpy2D(hdr.data(), 32, packs, (size_t)stride, 32, G, hipMemcpyDeviceToHost));
    std::vector<long long> an(G + 1, 1), zn(G + 1, c->rt_nz0);
    for (int r = 0; r < G; ++r) {
        if (hdr[4 * r] < 0 || hdr[4 * r + 3] != m || hdr[4 * r + 2] > stride)
            return fail(TWOSD_E_ARG, "refresh_assemble: pack %d is not a pack of this template", r);
        an[r + 1] = an[r] + hdr[4 * r];
        zn[r + 1] = zn[r] + hdr[4 * r + 1];
    }
    const long long nsrc = an[G], nzg = zn[G];
    if (nsrc > INT32_MAX / std::max(m, 1)) return fail(TWOSD_E_UNSUPPORTED, "refresh_assemble: too many sources");
    for (int i = 0; i < R; ++i)
        if (order[i] < 1 || order[i] >= nsrc) return fail(TWOSD_E_ARG, "refresh_assemble: source %d outside [1, %lld)", order[i], nsrc);
    if ((rc = c->d_gs_heads.reserve((size_t)std::max<long long>(nsrc - 1, 1) * m)) ||
        (rc = c->d_gs_cnt.reserve(PgTable::cnt_size((int)nsrc, m))) || (rc = c->d_gs_tot.reserve(PgTable::tot_size((int)nsrc))) ||
        (rc = c->d_gs_valid.reserve((size_t)nsrc)) || (rc = c->d_gs_ioff.reserve((size_t)nsrc)) ||
        (rc = c->d_gs_irow.reserve((size_t)nzg)) || (rc = c->d_gs_ival.reserve((size_t)nzg)))
        return rc;
    // the table: source 0 = this rank's primary (local compute row 0), then every rank's pack
    const PgTable T = pg_gathered_table(c, (int)nsrc), T0 = pg_local_table(c, c->rt_nsrc_local);
    std::vector<CopySeg> seg;
    for (int f = 0; f < 4; ++f) add_seg(seg, T0.plane(f, m), T.plane(f, m), sizeof(int) * m);
    add_seg(seg, T0.tot, T.tot, sizeof(int) * 4);
    add_seg(seg, T0.nztot(), T.nztot(), sizeof(int));
    add_seg(seg, T0.valid, T.valid, sizeof(int));
    add_seg(seg, T0.irow, T.irow, sizeof(int) * c->rt_nz0);
    add_seg(seg, T0.ival, T.ival, sizeof(double) * c->rt_nz0);
    for (int r = 0; r < G; ++r) {
        const long long n = hdr[4 * r], nz = hdr[4 * r + 1];
        const char *P = packs + (size_t)r * stride;
        rt_sections(T, m, an[r], n, zn[r], nz, rt_layout(n, nz, m), [&](void *t, size_t at, size_t bytes) { add_seg(seg, P + at, t, bytes); });
    }
    if ((rc = rt_copy(c, seg))) return rc;
    if (dbg) fprintf(stderr, "refresh_assemble: %lld sources, %lld entries, unpack %.2f ms\n", nsrc, nzg, ms_between(t0, Clock::now()));
    // host copy of the gathered table: tot (4 nsrc), nztot (nsrc) as they lie on the device, then valid
    int *h_tot = c->stage[STG_PG_TOT].reserve<int>((size_t)6 * nsrc);
    long long *h_ioff = c->stage[STG_PG_IOFF].reserve<long long>((size_t)nsrc);
    if (!h_tot || !h_ioff) return fail(TWOSD_E_DEVICE, "refresh: pinned staging allocation failed");
    int *h_nz = h_tot + 4 * nsrc, *h_valid = h_tot + 5 * nsrc;
    HIPCHK(hipMemcpyAsync(h_tot, T.tot, sizeof(int) * 5 * nsrc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(h_valid, T.valid, sizeof(int) * nsrc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    long long z = 0;
    for (long long a = 0; a < nsrc; ++a) {
        h_ioff[a] = z;
        z += h_nz[a];
    }
    if (z != nzg) return fail(TWOSD_E_ARG, "refresh_assemble: packs inconsistent (%lld vs %lld entries)", z, nzg);
    HIPCHK(hipMemcpyAsync(T.ioff, h_ioff, sizeof(long long) * nsrc, hipMemcpyHostToDevice, c->stream));
    // source table of the gathered build (template fields as the local compute)
    PgArgs A;
    if ((rc = pg_args(c, c->rt_nsrc_local, A))) return rc;
    pg_bind(A, T);
    // R == 0 (no rank had an optimal training scenario, or max_pool <= 1): the current pool stays,
    // as in twosd_pool_refresh (falling back to the primary basis alone costs ~90 pivots a scenario)
    if (R > 0) {
        std::vector<int> ord(R + 1);
        ord[0] = 0;
        std::copy(order, order + R, ord.begin() + 1);
        if ((rc = pg_assemble(c, A, PgHost{h_tot, h_valid, h_ioff, nzg}, ord, dbg)) != 0)
            return rc < 0 ? rc : fail(TWOSD_E_STATE, "refresh_assemble: the primary basis failed the device checks");
    } else {
        c->prep_valid = false;   // the selection box below changes
    }
    // selection box: the union of the ranks' training boxes
    if (c->k > 0) {
        c->sel_lo.assign(box_lo, box_lo + c->k);
        c->sel_hi.assign(box_hi, box_hi + c->k);
        c->sel_box = BoxCache{};   // not the single-rank cache
    }
    c->rt_nown = -1;
    c->rt_trained = false;
    const double ms = ms_between(t0, Clock::now());
    c->last_refresh_ms[3] = ms;
    c->last_refresh_ms[4] = c->last_refresh_ms[0] + c->last_refresh_ms[1] + c->last_refresh_ms[2] + ms;
    if (pool_size) *pool_size = (int)c->bp.bases.size();
    return TWOSD_OK;
}

extern "C" int twosd_last_refresh_ms(twosd_ctx *c, double *ms5) {
    if (!c || !ms5) return fail(TWOSD_E_ARG, "last_refresh_ms: NULL");
    for (int i = 0; i < 5; ++i) ms5[i] = c->last_refresh_ms[i];
    return TWOSD_OK;
}

// The global basis selection of a distributed refresh (host, no context): the bases the ranks
// list (concatenated in rank order), a key seen by several ranks counting the sum of its counts
// and owned by its first occurrence; the max_pool - 1 largest totals, ties by first occurrence --
// the single-rank refresh's stable sort over all training scenarios.
extern "C" int twosd_select_refresh_bases(const uint64_t *keys, const int64_t *counts, const int64_t *reps, const int32_t *rank_of,
                                          int n, int max_pool, int64_t *owner, int64_t *rep, int *npick) {
    if (n < 0 || !npick || (n > 0 && (!keys || !counts || !reps || !rank_of))) return fail(TWOSD_E_ARG, "select_refresh_bases: bad arguments");
    *npick = 0;
    if (n == 0 || max_pool <= 1) return TWOSD_OK;
    if (!owner || !rep) return fail(TWOSD_E_ARG, "select_refresh_bases: NULL output");
    std::vector<int> idx(n);
    for (int i = 0; i < n; ++i) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](int a, int b) { return keys[a] != keys[b] ? keys[a] < keys[b] : a < b; });
    struct G { int64_t tot; int first; };
    std::vector<G> g;
    g.reserve(n);
    for (int a = 0; a < n;) {
        int b = a;
        int64_t t = 0;
        while (b < n && keys[idx[b]] == keys[idx[a]]) t += counts[idx[b++]];
        g.push_back({t, idx[a]});   // the lowest index of the key: its first occurrence
        a = b;
    }
    const size_t k = std::min<size_t>(g.size(), (size_t)max_pool - 1);
    std::partial_sort(g.begin(), g.begin() + k, g.end(),
                      [](const G &a, const G &b) { return a.tot != b.tot ? a.tot > b.tot : a.first < b.first; });
    for (size_t i = 0; i < k; ++i) {
        owner[i] = rank_of[g[i].first];
        rep[i] = reps[g[i].first];
    }
    *npick = (int)k;
    return TWOSD_OK;
}
