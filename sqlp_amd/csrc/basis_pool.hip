// basis_pool.hip -- the warm-start basis pool (BasisPool, basis_pool.h): its bases in their host
// forms (validated heads, B^{-1} rows, pi0; lazily read back for a device-built pool), the
// pool-strided device arrays and their upload, the transitions that say what a change of the
// pool invalidates, and the ABI calls that install, extend and read it (twosd_compute_basis /
// set_basis / get_basis, twosd_pool_add_basis / pool_size / pool_get / pool_build).  The element
// rows and the per-x preparation are pool_select.hip's, the refresh pool_refresh.hip's; both
// change the pool's flags only through the transitions here.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <thread>
#include <vector>
#include "twosd_internal.h"
#include "twosd_ctx.h"

using namespace twosd;

// ---- the one list of the pool arrays ---------------------------------------------------------
PoolArrays twosd::pool_arrays(const twosd_ctx *c) {
    const PoolDev &d = c->bp.d;
    return PoolArrays{d.hb0, d.basic0, d.bnnz, d.d0, d.bcp, d.bci, d.bcv, d.brptr, d.brcol, d.brval,
                      d.kp, d.ke, d.kraw, d.kslot, d.kix, d.kv};
}

int twosd::pool_reserve(twosd_ctx *c, int P, size_t nz, size_t kz, size_t ez) {
    PoolDev &d = c->bp.d;
    const int m = c->L.m, MP = c->MP;
    int rc;
    if ((rc = d.brptr.reserve((size_t)P * (MP + 1))) || (rc = d.brcol.reserve(nz)) ||
        (rc = d.brval.reserve(nz)) || (rc = d.bcp.reserve((size_t)P * (MP + 1))) ||
        (rc = d.bci.reserve(nz)) || (rc = d.bcv.reserve(nz)) ||
        (rc = d.kp.reserve((size_t)P * (m + 1))) || (rc = d.ke.reserve(kz)) ||
        (rc = d.kraw.reserve(kz)) || (rc = d.kslot.reserve((size_t)P * (c->R + 1))) ||
        (rc = d.kix.reserve(ez)) || (rc = d.kv.reserve(ez)) ||
        (rc = d.hb0.reserve((size_t)P * MP)) || (rc = d.basic0.reserve((size_t)P * 64)) ||
        (rc = d.bnnz.reserve((size_t)P)) || (rc = d.d0.reserve((size_t)P * 64 * c->CH)))
        return rc;
    return TWOSD_OK;
}

// ---- transitions -----------------------------------------------------------------------------
// The pool's dependants: the per-x preparation (prep_valid: x_B and the selection stream of every
// basis), the element rows (k_valid: d.k*), the two-level candidate lists (pool indices), the
// head cache (hb_valid) and the selection box (sel_lo / sel_hi / sel_box: the training box of the
// deltas, which belongs to a training range and not to the pool).

// upload_pool wrote the ten arrays of its own from the host forms.  Invalid: the per-x
// preparation and the candidate lists (other bases), and the element rows (they are built from
// the same host rows by prepare_elements, on the next prepare_x or by the caller).  The head
// cache is left alone: upload_pool materialised every head first (pool_host_rows), so no basis
// refers to it any more and its flag is not read until the next device install clears it.  The
// selection box is left alone: it describes scenarios, and the callers that change the
// training range (twosd_pool_build, the refresh) set it themselves; install_basis, which starts
// a new pool, clears it.
void twosd::pool_installed_from_host(twosd_ctx *c) {
    c->prep_valid = false;
    c->bp.k_valid = false;
    reset_candidates(c);   // candidate lists refer to pool indices: rebuild after a change
}

// A device refresh filled all sixteen arrays with P bases (pg_fill_kernel): bases[0] keeps its
// host forms, bases[1, P) have none yet -- their heads are read from the head cache on first use
// (pool_head), their rows and pi0 from the arrays (pool_host_rows).  Invalid: the per-x
// preparation and the candidate lists (other bases), and the head cache (it holds the previous
// pool's d.hb0; nothing is copied here -- see pool_head).  Valid, unlike after a host install:
// the element rows, which the fill wrote with the rest.  The selection box is the refresh's own.
void twosd::pool_installed_from_device(twosd_ctx *c, int P) {
    c->bp.hb_valid = false;
    // host pool: the primary keeps its host forms; the new bases refer to their head rows
    std::vector<PoolBasis> keep(P);
    keep[0] = std::move(c->bp.bases[0]);
    for (int p = 1; p < P; ++p) {
        keep[p].hb_row = p;
        keep[p].dev_only = true;
    }
    c->bp.bases.swap(keep);
    std::thread([old = std::move(keep)]() mutable { old.clear(); }).detach();
    c->prep_valid = false;
    c->bp.k_valid = true;
    reset_candidates(c);
}

// The pool no longer matches the device arrays (a failed build or head read-back): keep only
// the primary basis (a host basis) and refuse solves until a basis is installed again.  Invalid:
// everything that describes the arrays -- has_basis, the per-x preparation, the element rows, the
// head cache (the failing path may have reallocated or overwritten it) and the candidate lists.
// The selection box stays: every call that would read it is refused without a basis, and the
// install_basis that ends that state clears it.
int twosd::pool_dropped(twosd_ctx *c, int code) {
    if (c->bp.bases.size() > 1) c->bp.bases.resize(1);
    c->bp.has_basis = false;
    c->prep_valid = false;
    c->bp.k_valid = false;
    c->bp.hb_valid = false;
    reset_candidates(c);
    return code;
}

// prepare_elements wrote d.k* for the current bases and positions
void twosd::pool_elements_ready(twosd_ctx *c) { c->bp.k_valid = true; }

// The element rows are B_p^{-1}[:, row_e] over the positions e, and the per-x preparation is built
// from them: both are stale.  The bases, their arrays and the candidate lists do not depend on the
// positions and stay.
void twosd::pool_positions_changed(twosd_ctx *c) {
    c->prep_valid = false;
    c->bp.k_valid = false;
}

// ---- lazy host forms -------------------------------------------------------------------------
// head of pool basis p into *h (materialised from c->bp.hb for a device-built basis on first
// use: a refresh of 4096 bases would otherwise spend ~2 ms building host heads nobody reads).
// A failed device read-back drops the pool (pool_dropped) and returns TWOSD_E_DEVICE.
int twosd::pool_head(twosd_ctx *c, int p, const std::vector<int> **h) {
    PoolBasis &B = c->bp.bases[p];
    if (B.hb_row >= 0 && !c->bp.hb_valid) {
        // the heads of a device-built pool are fetched on the first host use, not by the refresh
        // (at N = 8 every rank would copy 9 MB per step that only tests and the CPU baseline read)
        const size_t need = c->bp.bases.size() * (size_t)c->MP;
        if (!c->bp.hb.reserve<int>(need))
            return pool_dropped(c, fail(TWOSD_E_DEVICE, "pool heads: pinned allocation of %zu ints failed", need));
        hipError_t e = hipMemcpyAsync(c->bp.hb.p, c->bp.d.hb0, sizeof(int) * need, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return pool_dropped(c, fail(TWOSD_E_DEVICE, "pool heads: read-back failed: %s", hipGetErrorString(e)));
        c->bp.hb_valid = true;
    }
    if (B.hb_row >= 0) {
        const int m = c->L.m;
        const int *r = c->bp.hb.as<int>() + (size_t)B.hb_row * c->MP;
        B.head.resize(m);
        for (int i = 0; i < m; ++i) B.head[i] = r[i] >> 2;
        B.hb_row = -1;
    }
    if (h) *h = &B.head;
    return TWOSD_OK;
}
static int materialize_heads(twosd_ctx *c) {
    for (int p = 0; p < (int)c->bp.bases.size(); ++p)
        if (int rc = pool_head(c, p, nullptr)) return rc;
    return TWOSD_OK;
}

// validate a basis head (valid distinct columns, nonsingular, dual feasible for q) and
// compute its inverse; thread-safe, returns nullptr or the reason it was rejected
static const char *compute_pool_basis(const twosd_ctx *c, const std::vector<int> &head, PoolBasis &pb) {
    const HostLP &L = c->L;
    const int m = L.m, n = L.n;
    std::vector<char> seen(n + m, 0);
    for (int i = 0; i < m; ++i) {
        if (head[i] < 0 || head[i] >= n + m || seen[head[i]]) return "basis head has an invalid or duplicate column";
        seen[head[i]] = 1;
    }
    std::vector<double> B;
    basis_matrix(L, head, B);
    if (!dense_inverse(m, B, pb.Binv)) return "basis matrix is singular";
    const double dinf = basis_dual_infeasibility(L, head, pb.Binv, pb.pi0);
    if (dinf > 1e-7) return "basis is not dual feasible";
    pb.head = head;
    double amax = 0.0;
    for (double v : pb.Binv) amax = std::max(amax, std::fabs(v));
    const double drop = 1e-14 * amax;
    pb.rptr.assign(1, 0);
    pb.rcol.clear(); pb.rval.clear();
    for (int i = 0; i < m; ++i) {
        for (int cc = 0; cc < m; ++cc) {
            const double v = pb.Binv[(size_t)i * m + cc];
            if (std::fabs(v) > drop) { pb.rcol.push_back(cc); pb.rval.push_back(v); }
        }
        pb.rptr.push_back((int)pb.rcol.size());
    }
    return nullptr;
}
static int make_pool_basis(twosd_ctx *c, const std::vector<int> &head, PoolBasis &pb) {
    const char *why = compute_pool_basis(c, head, pb);
    return why ? fail(TWOSD_E_ARG, "%s", why) : TWOSD_OK;
}

// pi0 = c_B' B^{-1} from the CSR rows (rows ascending)
void twosd::pi0_from_rows(const twosd_ctx *c, PoolBasis &B) {
    const HostLP &L = c->L;
    const int m = L.m, n = L.n;
    B.pi0.assign(m, 0.0);
    for (int i = 0; i < m; ++i) {
        const int j = B.head[i];
        const double cb = j < n ? L.q[j] : 0.0;
        if (cb == 0.0) continue;
        for (int q = B.rptr[i]; q < B.rptr[i + 1]; ++q) B.pi0[B.rcol[q]] += cb * B.rval[q];
    }
}

// host CSR rows and pi0 of the bases a device refresh built (dev_only), read back from the
// pool arrays: upload_pool, prepare_elements and the host compose work on the host forms
int twosd::pool_host_rows(twosd_ctx *c) {
    if (int rc = materialize_heads(c)) return rc;
    const int P = (int)c->bp.bases.size(), MP = c->MP, m = c->L.m;
    int last = -1;
    for (int p = 0; p < P; ++p)
        if (c->bp.bases[p].dev_only) last = p;
    if (last < 0) return TWOSD_OK;
    const int Pd = last + 1;
    std::vector<int> rp((size_t)Pd * (MP + 1));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(rp.data(), c->bp.d.brptr, sizeof(int) * rp.size(), hipMemcpyDeviceToHost));
    size_t nz = 0;
    for (int p = 0; p < Pd; ++p) nz = std::max(nz, (size_t)rp[(size_t)p * (MP + 1) + m]);
    std::vector<int> col(std::max<size_t>(nz, 1));
    std::vector<double> val(std::max<size_t>(nz, 1));
    if (nz) {
        HIPCHK(hipMemcpy(col.data(), c->bp.d.brcol, sizeof(int) * nz, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(val.data(), c->bp.d.brval, sizeof(double) * nz, hipMemcpyDeviceToHost));
    }
    parallel_for(Pd, [&](int p) {
        PoolBasis &B = c->bp.bases[p];
        if (!B.dev_only) return;
        const int *r = rp.data() + (size_t)p * (MP + 1);
        B.rptr.resize(m + 1);
        for (int i = 0; i <= m; ++i) B.rptr[i] = r[i] - r[0];
        B.rcol.assign(col.begin() + r[0], col.begin() + r[m]);
        B.rval.assign(val.begin() + r[0], val.begin() + r[m]);
        pi0_from_rows(c, B);
        B.dev_only = false;
    });
    return TWOSD_OK;
}

// the host compose of a refresh: the bases become the primary followed by the fresh[a] with
// ok[a], all in host form.  The arrays do not hold them until the caller's upload_pool.
void twosd::pool_replace_host_bases(twosd_ctx *c, std::vector<PoolBasis> &fresh, const std::vector<char> &ok) {
    std::vector<PoolBasis> keep;
    keep.reserve(fresh.size() + 1);
    keep.push_back(std::move(c->bp.bases[0]));   // the primary basis stays bases[0]
    for (size_t a = 0; a < fresh.size(); ++a)
        if (ok[a]) keep.push_back(std::move(fresh[a]));
    c->bp.bases.swap(keep);
    // the old pool's host data is released on a helper thread (thousands of vectors)
    std::thread([old = std::move(keep)]() mutable { old.clear(); }).detach();
}

// Upload the hypersparse-kernel form of every pool basis, pool-strided (bases[0] first, so
// the leading MP / 64 / 64C entries are the primary basis): hb0 (MP), basic0 (64),
// d0 (64C), B^{-1} columns as CSC (bcp absolute into the concatenated bci/bcv),
// B^{-1} rows as CSR (brptr absolute into the concatenated brcol/brval).
int twosd::upload_pool(twosd_ctx *c) {
    const auto t_up0 = std::chrono::steady_clock::now();
    if (int rc0 = pool_host_rows(c)) return rc0;
    const HostLP &L = c->L;
    const int m = L.m, n = L.n, MP = c->MP, P = (int)c->bp.bases.size();
    std::vector<int8_t> bt(n + m);
    HIPCHK(hipMemcpy(bt.data(), c->d_btype, n + m, hipMemcpyDeviceToHost));
    std::vector<int> hb((size_t)P * MP), bnnz(P, 0);
    std::vector<uint64_t> basic((size_t)P * 64);
    // B^{-1} of every basis by rows (CSR) and by columns (CSC, rows ascending), both at the same
    // per-basis offset ro[p]; offsets are known up front, so every basis fills its part of the
    // concatenated arrays directly (default-initialised buffers, first touch in parallel)
    std::vector<size_t> ro(P + 1, 0);
    for (int p = 0; p < P; ++p) ro[p + 1] = ro[p] + c->bp.bases[p].rcol.size();
    if (ro[P] > INT32_MAX) return fail(TWOSD_E_UNSUPPORTED, "basis pool too large (> 2^31 entries)");
    const size_t nz = std::max<size_t>(ro[P], 1);
    std::vector<int> rp_all((size_t)P * (MP + 1)), cp_all((size_t)P * (MP + 1));
    int *rc_all = c->stage[STG_POOL_RCOL].reserve<int>(nz), *ci_all = c->stage[STG_POOL_CROW].reserve<int>(nz);
    double *rv_all = c->stage[STG_POOL_RVAL].reserve<double>(nz), *cv_all = c->stage[STG_POOL_CVAL].reserve<double>(nz);
    double *d0_all = c->stage[STG_POOL_D0].reserve<double>((size_t)P * 64 * std::max(c->CH, 1));
    if (!rc_all || !ci_all || !rv_all || !cv_all || !d0_all) return fail(TWOSD_E_DEVICE, "pool upload: pinned staging allocation failed");
    parallel_for(P, [&](int p) {
        const PoolBasis &B = c->bp.bases[p];
        bnnz[p] = (int)B.rcol.size();
        const size_t pp = (size_t)p, base = ro[p];
        pool_pack_basis(L, bt.data(), B, MP, c->CH, (int)base,
                        PoolPackOut{hb.data() + pp * MP, basic.data() + pp * 64, rp_all.data() + pp * (MP + 1), rc_all + base,
                                    rv_all + base, cp_all.data() + pp * (MP + 1), ci_all + base, cv_all + base,
                                    d0_all + pp * 64 * std::max(c->CH, 0)});
    });
    const auto tc = std::chrono::steady_clock::now();
    PoolDev &d = c->bp.d;
    int rc;
    if ((rc = d.hb0.upload_reserve(hb)) || (rc = d.basic0.upload_reserve(basic)) || (rc = d.bnnz.upload_reserve(bnnz))) return rc;
    if (c->CH > 0 &&
        ((rc = d.bcp.upload_reserve(cp_all)) || (rc = d.bci.upload_reserve(ci_all, ro[P])) ||
         (rc = d.bcv.upload_reserve(cv_all, ro[P])) || (rc = d.brptr.upload_reserve(rp_all)) ||
         (rc = d.brcol.upload_reserve(rc_all, ro[P])) || (rc = d.brval.upload_reserve(rv_all, ro[P])) ||
         (rc = d.d0.upload_reserve(d0_all, (size_t)P * 64 * c->CH))))
        return rc;
    if (getenv("TWOSD_DEBUG")) {
        const auto td = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "upload_pool P=%d: build %.1f ms, upload %.1f ms (%.1f MB, %zu nonzeros)\n", P, ms(t_up0, tc), ms(tc, td),
                (ro[P] * 24.0 + (size_t)P * 64 * std::max(c->CH, 0) * 8.0) / 1e6, ro[P]);
    }
    pool_installed_from_host(c);
    return TWOSD_OK;
}

static int install_basis(twosd_ctx *c, const std::vector<int> &head) {
    PoolBasis pb;
    int rc = make_pool_basis(c, head, pb);
    if (rc) return rc;
    c->bp.head0 = head;
    c->bp.bases.clear();
    c->sel_lo.clear();
    c->sel_hi.clear();
    c->sel_box = BoxCache{};
    c->bp.bases.push_back(std::move(pb));
    if ((rc = upload_pool(c))) return rc;
    c->bp.has_basis = true;
    return TWOSD_OK;
}

static bool same_basis(const std::vector<int> &a, const std::vector<int> &b) {
    std::vector<int> sa(a), sb(b);
    std::sort(sa.begin(), sa.end());
    std::sort(sb.begin(), sb.end());
    return sa == sb;
}

// append a basis to the pool; returns 1 if added, 0 if already present, < 0 on error
static int pool_add(twosd_ctx *c, const std::vector<int> &head, bool upload_now) {
    if (int rc = materialize_heads(c)) return rc;
    for (const PoolBasis &B : c->bp.bases)
        if (same_basis(B.head, head)) return 0;
    PoolBasis pb;
    int rc = make_pool_basis(c, head, pb);
    if (rc) return rc;
    std::vector<double>().swap(pb.Binv);
    c->bp.bases.push_back(std::move(pb));
    if (upload_now && (rc = upload_pool(c))) return rc;
    return 1;
}

extern "C" int twosd_compute_basis(twosd_ctx *c, const double *x, const double *values) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "compute_basis: no template");
    HIPCHK(hipSetDevice(c->device));
    std::vector<double> dv(c->k, 0.0);
    if (values)
        for (int e = 0; e < c->k; ++e) dv[e] = values[e] - template_value(c, e);
    std::vector<double> b;
    rhs_at(c, x, values ? dv.data() : nullptr, b);
    std::vector<int> head;
    double obj = 0;
    int iters = 0;
    std::string err;
    const int st = setup_solve(c->L, b, head, obj, iters, err);
    if (st != TWOSD_LP_OPTIMAL) return fail(TWOSD_E_LP, "compute_basis: %s (status %d)", err.c_str(), st);
    return install_basis(c, head);
}

extern "C" int twosd_set_basis(twosd_ctx *c, const int *head) {
    if (!c || !c->has_template || !head) return fail(TWOSD_E_STATE, "set_basis: no template / NULL head");
    HIPCHK(hipSetDevice(c->device));
    return install_basis(c, std::vector<int>(head, head + c->L.m));
}

extern "C" int twosd_get_basis(twosd_ctx *c, int *head) {
    if (!c || !c->bp.has_basis || !head) return fail(TWOSD_E_STATE, "get_basis: no basis");
    std::copy(c->bp.head0.begin(), c->bp.head0.end(), head);
    return TWOSD_OK;
}

extern "C" int twosd_pool_add_basis(twosd_ctx *c, const int *head, int *added) {
    if (!c || !c->bp.has_basis || !head) return fail(TWOSD_E_STATE, "pool_add_basis: no primary basis / NULL head");
    HIPCHK(hipSetDevice(c->device));
    const int rc = pool_add(c, std::vector<int>(head, head + c->L.m), true);
    if (rc < 0) return rc;
    if (added) *added = rc;
    return TWOSD_OK;
}

extern "C" int twosd_pool_size(twosd_ctx *c, int *size) {
    if (!c || !size) return fail(TWOSD_E_ARG, "pool_size: NULL argument");
    *size = (int)c->bp.bases.size();
    return TWOSD_OK;
}

extern "C" int twosd_pool_get(twosd_ctx *c, int p, int *head) {
    if (c && !c->bp.has_basis) return fail(TWOSD_E_STATE, "pool_get: no basis");
    if (!c || !head || p < 0 || p >= (int)c->bp.bases.size()) return fail(TWOSD_E_ARG, "pool_get: basis %d of %zu", p, c ? c->bp.bases.size() : 0);
    const std::vector<int> *h = nullptr;
    if (int rc = pool_head(c, p, &h)) return rc;
    std::copy(h->begin(), h->end(), head);
    return TWOSD_OK;
}

static int64_t pivots_of_last_lp(twosd_ctx *c, int N) {
    std::vector<int> its(N);
    if (hipMemcpy(its.data(), c->d_iters, sizeof(int) * N, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    int64_t sum = 0;
    for (int v : its) sum += v;
    return sum;
}

// Grow the pool from training scenarios [first, first + count) of epigraph epi at x.  The
// first half harvests: solved from the current pool, its optimal bases are added in order
// of decreasing frequency (ties: first occurrence) up to max_pool bases.  The second half
// validates: the grown pool is kept only if it solves those scenarios in fewer pivots.
extern "C" int twosd_pool_build(twosd_ctx *c, int epi, const double *x, int first, int count, int max_pool,
                                int *pool_size) {
    if (!c || !c->bp.has_basis) return fail(TWOSD_E_STATE, "pool_build: no primary basis");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "pool_build: epigraph %d does not exist", epi);
    const EpiDevice &E = c->epis[epi];
    if (first < 0 || count < 0 || first + count > E.count || max_pool < 1 || (c->n1 > 0 && !x))
        return fail(TWOSD_E_ARG, "pool_build: bad arguments");
    if (pool_select_lds_bytes(c->k) + 17 * 1024 > 160 * 1024)   // + the selection kernels' static LDS
        return fail(TWOSD_E_UNSUPPORTED, "pool_build: k = %d random elements too many for pool selection", c->k);
    HIPCHK(hipSetDevice(c->device));
    const int m = c->L.m;
    const int nh = count / 2, nv = count - nh;
    if (count > 0 && c->k > 0) {   // training box of the deltas (selection row pruning)
        if (int rc = training_box(c, E, epi, first, count, c->sel_lo, c->sel_hi, nullptr)) return rc;
        c->sel_box = BoxCache{};   // the refresh's cached box no longer applies
        c->prep_valid = false;
    }
    if (nh > 0 && (int)c->bp.bases.size() < max_pool) {
        const double *dh = E.d_dv + (size_t)first * c->k, *dval = dh + (size_t)nh * c->k;
        int rc;
        if ((rc = run_lp(c, x, dval, nv))) return rc;
        const int64_t piv0 = pivots_of_last_lp(c, nv);
        LpRun harvest;
        harvest.want_head = true;
        if ((rc = run_lp(c, x, dh, nh, harvest))) return rc;
        std::vector<int> heads((size_t)nh * m), st(nh);
        HIPCHK(hipMemcpy(heads.data(), c->d_head_out, sizeof(int) * heads.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(st.data(), c->d_status, sizeof(int) * nh, hipMemcpyDeviceToHost));
        std::map<std::vector<int>, std::pair<int, int>> freq;   // sorted head -> (count, first scenario)
        if ((rc = materialize_heads(c))) return rc;
        for (const PoolBasis &B : c->bp.bases) {
            std::vector<int> key(B.head);
            std::sort(key.begin(), key.end());
            freq[key] = {0, -1};                                 // already in the pool
        }
        for (int s = 0; s < nh; ++s) {
            if (st[s] != TWOSD_LP_OPTIMAL) continue;
            std::vector<int> key(heads.begin() + (size_t)s * m, heads.begin() + (size_t)(s + 1) * m);
            std::sort(key.begin(), key.end());
            auto it = freq.find(key);
            if (it == freq.end()) freq.emplace(std::move(key), std::make_pair(1, s));
            else if (it->second.second >= 0) ++it->second.first;
        }
        std::vector<std::pair<int, int>> order;   // (-count, first scenario)
        for (auto &kv : freq)
            if (kv.second.second >= 0) order.push_back({-kv.second.first, kv.second.second});
        std::sort(order.begin(), order.end());
        const size_t old_size = c->bp.bases.size();
        // candidates are distinct and new; their inverses are computed in parallel, and a
        // candidate that fails validation (numerically singular / dual infeasible) is skipped
        const size_t want = std::min(order.size(), (size_t)max_pool - old_size);
        std::vector<PoolBasis> cand(want);
        std::vector<int> ok(want, 0);
        parallel_for((int)want, [&](int a) {   // threaded at any size: a dense m x m inverse each
            const int s = order[a].second;
            std::vector<int> head(heads.begin() + (size_t)s * m, heads.begin() + (size_t)(s + 1) * m);
            ok[a] = compute_pool_basis(c, head, cand[a]) == nullptr;
            std::vector<double>().swap(cand[a].Binv);   // sparse forms kept; dense m x m only for the primary
        }, 1);
        for (size_t a = 0; a < want; ++a)
            if (ok[a]) c->bp.bases.push_back(std::move(cand[a]));
        if (c->bp.bases.size() > old_size) {
            if ((rc = upload_pool(c))) return rc;
            if ((rc = run_lp(c, x, dval, nv))) return rc;
            const int64_t piv1 = pivots_of_last_lp(c, nv);
            std::vector<int> st2(nv);
            HIPCHK(hipMemcpy(st2.data(), c->d_status, sizeof(int) * nv, hipMemcpyDeviceToHost));
            const bool all_ok = std::all_of(st2.begin(), st2.end(), [](int v) { return v == TWOSD_LP_OPTIMAL; });
            if (piv1 < 0 || piv0 < 0 || piv1 >= piv0 || !all_ok) {   // no gain: back to the old pool
                c->bp.bases.resize(old_size);
                if ((rc = upload_pool(c))) return rc;
            }
        }
    }
    if (pool_size) *pool_size = (int)c->bp.bases.size();
    return TWOSD_OK;
}
