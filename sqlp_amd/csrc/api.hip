// api.hip -- C ABI of libtwosd_hip.so (declared in include/twosd_hip.h).
//
// Owns the device-resident state of the TwoSD hot path on one MI355X:
//   template (W CSC, q, bound types), shared warm-start basis (B0^{-1}, pi0), per-epigraph
//   scenario pools (deltas, weights), the dual vertex set, and the LP/cut workspaces.
// Every call is synchronous on the context's own HIP stream.
// Here: errors, create / destroy, canonical form, template, positions, epigraphs and scenarios,
// distributions, sampling plans.  The warm-start basis pool (host forms, upload, validity, the
// basis and pool calls of the ABI) is in basis_pool.hip, the per-x preparation and warm-start
// selection in pool_select.hip, the LP launch with its outputs and solve_* in lp_batch.hip,
// out-of-sample evaluation in evaluate.hip, the pool refresh in pool_refresh.hip.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <memory>
#include "twosd_internal.h"
#include "twosd_ctx.h"

using namespace twosd;

static thread_local std::string g_err;

int twosd::fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char *twosd_last_error(void) { return g_err.c_str(); }
extern "C" const char *twosd_version(void) { return "twosd-mi355x 0.1 (gfx950)"; }

extern "C" int twosd_create(int device, twosd_ctx **out) {
    if (!out) return fail(TWOSD_E_ARG, "twosd_create: out is NULL");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(TWOSD_E_ARG, "twosd_create: device %d of %d", device, ndev);
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<twosd_ctx> c(new twosd_ctx());   // a failure below destroys what was created
    c->device = device;
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : c->ev) HIPCHK(hipEventCreate(&e));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    c->num_cus = prop.multiProcessorCount;
    const char *km = getenv("TWOSD_KMAX");
    if (km) c->kmax_override = atoi(km);
    *out = c.release();
    return TWOSD_OK;
}

// a template re-set starts from the state of a fresh context: buffers, flags and statistics
static void free_template(twosd_ctx *c) { static_cast<TemplateState &>(*c) = TemplateState(); }

extern "C" int twosd_destroy(twosd_ctx *c) {
    if (!c) return TWOSD_OK;
    hipSetDevice(c->device);
    delete c;
    return TWOSD_OK;
}

// ---- general stage-2 bounds: canonical form ------------------------------------------------
// min q'y, W y (senses) b, lo <= y <= hi  ->  min q'y' + c0, W' y' (senses') b', y' >= 0, per column
// (lo, hi):  [0, inf) kept;  [lo, inf) y = lo + y';  (-inf, hi] y = hi - y' (column and cost
// negated);  free y = y+ - y- (the y- columns appended after the kept ones, ascending j);
// lo = hi: the column leaves the LP;  [lo, hi] y = lo + y' plus one L row y' <= hi - lo (appended
// after the m2 rows, ascending j).  s is the shift point (lo, hi of the negated kind, or 0):
// r' = r - W s over the columns with s != 0 in ascending j, entries in CSC order; c0 = q.s likewise.
// A dual of the canonical LP is the m2 row duals followed by one multiplier <= 0 per boxed
// variable; the unbounded kinds need none (their dual constraint is the LP's own column).
namespace {
struct Canon {
    bool any = false;             // false: every bound is [0, +inf), the arrays below are the input's
    int m_lp = 0, n_lp = 0, nb = 0;
    std::vector<int> colptr, rowidx;
    std::vector<double> val, q, r;
    std::vector<char> sense;
    double c0 = 0.0;
    // back-map of caller column j: y_j = off[j] + sign[j] * y'[src[j]] - y'[src2[j]] (src / src2 = -1: term absent)
    std::vector<int> src, src2, box_col;
    std::vector<double> sign, off;
};
}  // namespace

// W: m2 x n2 CSC, 0-based; ylb / yub nullable (0 / +inf)
static int canonical_form_impl(int m2, int n2, const int *cp, const int *ri, const double *v, const double *q,
                               const double *r, const char *sense, const double *ylb, const double *yub, Canon &K) {
    enum { KEEP, SHIFT, NEG, FREE, FIXED, BOX };
    std::vector<int> kind(n2, KEEP);
    std::vector<double> s(n2, 0.0);
    K = Canon();
    int nfree = 0, nfixed = 0;
    for (int j = 0; j < n2; ++j) {
        const double lo = ylb ? ylb[j] : 0.0, hi = yub ? yub[j] : INFINITY;
        if (std::isnan(lo) || std::isnan(hi) || lo > hi || lo == INFINITY || hi == -INFINITY)
            return fail(TWOSD_E_ARG, "y[%d] bounds [%g, %g] are not an interval", j, lo, hi);
        const bool flo = std::isfinite(lo), fhi = std::isfinite(hi);
        if (flo && !fhi) kind[j] = lo == 0.0 ? KEEP : SHIFT;
        else if (!flo && fhi) kind[j] = NEG;
        else if (!flo && !fhi) kind[j] = FREE;
        else kind[j] = lo == hi ? FIXED : BOX;
        s[j] = kind[j] == NEG ? hi : (flo ? lo : 0.0);
        if (kind[j] == KEEP) s[j] = 0.0;
        K.any |= kind[j] != KEEP;
        K.nb += kind[j] == BOX;
        nfree += kind[j] == FREE;
        nfixed += kind[j] == FIXED;
    }
    K.src.assign(n2, -1); K.src2.assign(n2, -1);
    K.sign.assign(n2, 1.0); K.off.assign(n2, 0.0);
    K.m_lp = m2 + K.nb;
    K.n_lp = n2 - nfixed + nfree;
    K.r.assign(r, r + m2);
    K.sense.assign(sense, sense + m2);
    if (!K.any) {
        K.colptr.assign(cp, cp + n2 + 1);
        K.rowidx.assign(ri, ri + cp[n2]);
        K.val.assign(v, v + cp[n2]);
        K.q.assign(q, q + n2);
        for (int j = 0; j < n2; ++j) K.src[j] = j;
        return TWOSD_OK;
    }
    // r' = r - W s and c0 = q.s, columns ascending
    for (int j = 0; j < n2; ++j) {
        if (s[j] == 0.0) continue;
        for (int p = cp[j]; p < cp[j + 1]; ++p) K.r[ri[p]] -= v[p] * s[j];
        K.c0 += q[j] * s[j];
    }
    K.colptr.assign(1, 0);
    int col = 0, box = 0;
    for (int j = 0; j < n2; ++j) {
        K.off[j] = s[j];
        if (kind[j] == FIXED) continue;
        const double sg = kind[j] == NEG ? -1.0 : 1.0;
        K.src[j] = col++;
        K.sign[j] = sg;
        for (int p = cp[j]; p < cp[j + 1]; ++p) { K.rowidx.push_back(ri[p]); K.val.push_back(sg * v[p]); }
        if (kind[j] == BOX) {
            K.rowidx.push_back(m2 + box); K.val.push_back(1.0);
            K.r.push_back((yub ? yub[j] : INFINITY) - (ylb ? ylb[j] : 0.0));
            K.sense.push_back('L');
            K.box_col.push_back(j);
            ++box;
        }
        K.q.push_back(sg * q[j]);
        K.colptr.push_back((int)K.rowidx.size());
    }
    for (int j = 0; j < n2; ++j) {   // y- of the free columns
        if (kind[j] != FREE) continue;
        K.src2[j] = col++;
        for (int p = cp[j]; p < cp[j + 1]; ++p) { K.rowidx.push_back(ri[p]); K.val.push_back(-v[p]); }
        K.q.push_back(-q[j]);
        K.colptr.push_back((int)K.rowidx.size());
    }
    return TWOSD_OK;
}

// W CSC of the caller (index base `base`) as 0-based ints, validated
static int read_csc(int m2, int n2, const int64_t *Wcp, const int64_t *Wrv, const double *Wnz, int base, std::vector<int> &cp,
                    std::vector<int> &ri, std::vector<double> &v) {
    cp.resize(n2 + 1);
    for (int j = 0; j <= n2; ++j) {
        cp[j] = (int)(Wcp[j] - base);
        if (j && cp[j] < cp[j - 1]) return fail(TWOSD_E_ARG, "W colptr malformed");
    }
    const int nnzW = cp[n2];
    if (cp[0] != 0 || nnzW < 0) return fail(TWOSD_E_ARG, "W colptr malformed");
    ri.resize(nnzW); v.resize(nnzW);
    for (int p = 0; p < nnzW; ++p) {
        ri[p] = (int)(Wrv[p] - base);
        v[p] = Wnz[p];
        if (ri[p] < 0 || ri[p] >= m2) return fail(TWOSD_E_ARG, "W row index %d out of range", ri[p] + base);
    }
    return TWOSD_OK;
}

extern "C" int twosd_canonical_form(int m2, int n2, const int64_t *Wcp, const int64_t *Wrv, const double *Wnz, const double *q,
                                    const double *r, const char *sense, const double *ylb, const double *yub, int base,
                                    int *m_lp, int *n_lp, int *n_bound_rows, int64_t *out_colptr, int64_t *out_rowval,
                                    double *out_nzval, double *out_q, double *out_r, char *out_sense, double *c0,
                                    int *col_src, double *col_sign, double *col_off, int *col_src2, int *box_col) {
    if (m2 <= 0 || n2 <= 0 || !Wcp || !Wrv || !Wnz || !q || !r || !sense || !m_lp || !n_lp || !n_bound_rows)
        return fail(TWOSD_E_ARG, "twosd_canonical_form: bad sizes or NULL arrays");
    if (base != 0 && base != 1) return fail(TWOSD_E_ARG, "index_base must be 0 or 1");
    std::vector<int> cp, ri;
    std::vector<double> v;
    int rc;
    if ((rc = read_csc(m2, n2, Wcp, Wrv, Wnz, base, cp, ri, v))) return rc;
    Canon K;
    if ((rc = canonical_form_impl(m2, n2, cp.data(), ri.data(), v.data(), q, r, sense, ylb, yub, K))) return rc;
    *m_lp = K.m_lp; *n_lp = K.n_lp; *n_bound_rows = K.nb;
    if (out_colptr) for (int j = 0; j <= K.n_lp; ++j) out_colptr[j] = K.colptr[j] + base;
    if (out_rowval) for (size_t p = 0; p < K.rowidx.size(); ++p) out_rowval[p] = K.rowidx[p] + base;
    if (out_nzval) std::copy(K.val.begin(), K.val.end(), out_nzval);
    if (out_q) std::copy(K.q.begin(), K.q.end(), out_q);
    if (out_r) std::copy(K.r.begin(), K.r.end(), out_r);
    if (out_sense) std::copy(K.sense.begin(), K.sense.end(), out_sense);
    if (c0) *c0 = K.c0;
    for (int j = 0; j < n2; ++j) {
        if (col_src) col_src[j] = K.src[j] < 0 ? -1 : K.src[j] + base;
        if (col_src2) col_src2[j] = K.src2[j] < 0 ? -1 : K.src2[j] + base;
        if (col_sign) col_sign[j] = K.sign[j];
        if (col_off) col_off[j] = K.off[j];
    }
    if (box_col) for (int b = 0; b < K.nb; ++b) box_col[b] = K.box_col[b] + base;
    return TWOSD_OK;
}

extern "C" int twosd_lp_shape(twosd_ctx *c, int *m_lp, int *n_lp, int *n_bound_rows) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "lp_shape: no template");
    if (m_lp) *m_lp = c->L.m;
    if (n_lp) *n_lp = c->L.n;
    if (n_bound_rows) *n_bound_rows = c->nb;
    return TWOSD_OK;
}

extern "C" int twosd_set_template(twosd_ctx *c, int m2, int n1, int n2, const int64_t *Tcp, const int64_t *Trv,
                                  const double *Tnz, const int64_t *Wcp, const int64_t *Wrv, const double *Wnz,
                                  const double *q, const double *r, const char *sense, const double *ylb,
                                  const double *yub, int base) {
    if (!c) return fail(TWOSD_E_ARG, "ctx is NULL");
    if (m2 <= 0 || n1 < 0 || n2 <= 0 || !Wcp || !Wrv || !Wnz || !q || !r || !sense || (n1 > 0 && (!Tcp || !Trv || !Tnz)))
        return fail(TWOSD_E_ARG, "twosd_set_template: bad sizes or NULL arrays");
    if (base != 0 && base != 1) return fail(TWOSD_E_ARG, "index_base must be 0 or 1");
    HIPCHK(hipSetDevice(c->device));
    free_template(c);
    HostLP &L = c->L;
    int rc;
    if ((rc = read_csc(m2, n2, Wcp, Wrv, Wnz, base, L.colptr, L.rowidx, L.val))) return rc;
    for (int i = 0; i < m2; ++i)
        if (sense[i] != 'G' && sense[i] != 'L' && sense[i] != 'E')
            return fail(TWOSD_E_ARG, "sense[%d] = '%c' (expected G/L/E)", i, sense[i]);
    // general bounds leave here: from this point m2 / n2 are the LP's sizes (the caller's when
    // every bound is [0, +inf), and then L holds the caller's arrays untouched)
    const int m2u = m2, n2u = n2;
    Canon K;
    if ((rc = canonical_form_impl(m2u, n2u, L.colptr.data(), L.rowidx.data(), L.val.data(), q, r, sense, ylb, yub, K))) return rc;
    c->has_bounds = K.any;
    c->m2_user = m2u; c->n2_user = n2u; c->nb = K.nb; c->c0 = K.c0;
    c->r_user.assign(r, r + m2u);
    if (K.any) {
        L.colptr.swap(K.colptr); L.rowidx.swap(K.rowidx); L.val.swap(K.val);
        m2 = K.m_lp; n2 = K.n_lp;
        if (n2 <= 0) return fail(TWOSD_E_UNSUPPORTED, "every stage-2 variable is fixed: no LP is left");
    }
    L.m = m2; L.n = n2;
    L.q.swap(K.q);
    L.sense.swap(K.sense);
    const int nnzW = L.colptr[n2];
    c->n1 = n1;
    c->r.swap(K.r);
    c->T.assign((size_t)m2 * n1, 0.0);   // dense T (LP rows x n1; the bound rows are zero) on the host for per-x setup
    for (int j = 0; j < n1; ++j)
        for (int64_t p = Tcp[j] - base; p < Tcp[j + 1] - base; ++p) {
            const int i = (int)(Trv[p] - base);
            if (i < 0 || i >= m2u) return fail(TWOSD_E_ARG, "T row index out of range");
            c->T[(size_t)i * n1 + j] = Tnz[p];
        }
    // the envelope applies to the LP's sizes; the messages name the caller's too
    char sizes[160];
    snprintf(sizes, sizeof sizes, "m2 = %d, n2 = %d (LP: %d rows with %d bound rows of boxed variables, %d columns)", m2u, n2u, m2,
             c->nb, n2);
    const int R = hyper_rows_per_lane(m2);
    if (R < 0) return fail(TWOSD_E_UNSUPPORTED, "%s: %d LP rows exceed the LP kernel envelope (%d rows)", sizes, m2, 64 * 16);
    const int C = (n2 + m2 + 63) / 64;
    if (C > kMaxColsPerLane)
        return fail(TWOSD_E_UNSUPPORTED, "%s: %d LP columns and rows exceed %d columns", sizes, n2 + m2, 64 * kMaxColsPerLane);
    c->R = R; c->MP = 64 * R; c->C = C;
    c->CH = hyper_cols_per_lane(n2 + m2);
    if (c->CH <= 0) return fail(TWOSD_E_UNSUPPORTED, "%s: %d LP columns and rows exceed the LP kernel's column slots", sizes, n2 + m2);
    // device template
    if (K.any && ((rc = c->d_bm_src.upload(K.src)) || (rc = c->d_bm_src2.upload(K.src2)) || (rc = c->d_bm_sign.upload(K.sign)) ||
                  (rc = c->d_bm_off.upload(K.off))))
        return rc;
    if ((rc = c->d_colptr.alloc(n2 + 1)) || (rc = c->d_rowidx.alloc(nnzW)) || (rc = c->d_val.alloc(nnzW)) ||
        (rc = c->d_q.alloc(n2)) || (rc = c->d_btype.alloc(n2 + m2)) || (rc = c->d_fixedmask.alloc(64)) ||
        (rc = c->d_ubmask.alloc(64)))
        return rc;
    std::vector<int8_t> bt(n2 + m2);
    std::vector<uint64_t> fixedm(64, 0), ubm(64, 0);
    for (int j = 0; j < n2 + m2; ++j) {
        int b = BT_Y;
        if (j >= n2) { char s = L.sense[j - n2]; b = s == 'G' ? BT_G : (s == 'L' ? BT_L : BT_E); }
        bt[j] = (int8_t)b;
    }
    for (int j = 0; j < 64 * 64; ++j) {
        const int lane = j & 63, cs = j >> 6;
        if (j >= n2 + m2 || bt[j] == BT_E) fixedm[lane] |= 1ull << cs;
        else if (bt[j] == BT_G) ubm[lane] |= 1ull << cs;
    }
    HIPCHK(hipMemcpy(c->d_colptr, L.colptr.data(), sizeof(int) * (n2 + 1), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_rowidx, L.rowidx.data(), sizeof(int) * std::max(nnzW, 1), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_val, L.val.data(), sizeof(double) * std::max(nnzW, 1), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_q, L.q.data(), sizeof(double) * n2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_btype, bt.data(), n2 + m2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_fixedmask, fixedm.data(), sizeof(uint64_t) * 64, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_ubmask, ubm.data(), sizeof(uint64_t) * 64, hipMemcpyHostToDevice));
    if (c->CH > 0) {   // W by rows (CSR, columns ascending) for the row-wise pricing scatter
        std::vector<std::vector<std::pair<int, double>>> rows(m2);
        for (int j = 0; j < n2; ++j)
            for (int p = L.colptr[j]; p < L.colptr[j + 1]; ++p) rows[L.rowidx[p]].push_back({j, L.val[p]});
        std::vector<int> cp(m2 + 1, 0), cc;
        std::vector<double> cv;
        for (int i = 0; i < m2; ++i) {
            for (auto &e : rows[i]) { cc.push_back(e.first); cv.push_back(e.second); }
            cp[i + 1] = (int)cc.size();
        }
        if ((rc = c->d_wcp.upload(cp)) || (rc = c->d_wcc.upload(cc)) || (rc = c->d_wcv.upload(cv))) return rc;
    }
    c->has_template = true;
    c->k = 0;
    c->pos_row.clear(); c->pos_col.clear();
    if ((rc = dvs_init(c))) return rc;
    return TWOSD_OK;
}

extern "C" int twosd_set_random_positions(twosd_ctx *c, int k, const int *row, const int *col, int base) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "set_random_positions: no template");
    if (k < 0 || (k > 0 && (!row || !col))) return fail(TWOSD_E_ARG, "set_random_positions: bad arguments");
    for (auto &e : c->epis)
        if (e.count) return fail(TWOSD_E_STATE, "set_random_positions: epigraphs already hold scenarios");
    // checked into a copy first: a refused call leaves k and the positions as they were
    std::vector<int> pr(k), pc(k);
    for (int e = 0; e < k; ++e) {
        const int rr = row[e] - base;
        const int cc = col[e] < 0 ? -1 : col[e] - base;
        if (rr < 0 || rr >= c->m2_user) return fail(TWOSD_E_ARG, "position %d: row %d out of range", e, row[e]);   // not a bound row
        if (cc >= c->n1) return fail(TWOSD_E_ARG, "position %d: column %d is not a first-stage column (KeyError in delta_coefficients, subprob.jl:116)", e, col[e]);
        // a position listed twice: the reference keeps the last write (delta_rhs[row] = ..., subprob.jl:114-117),
        // every kernel here would add both deltas; refused (k <= 127 for the cut, so the scan is short)
        for (int d = 0; d < e; ++d)
            if (pr[d] == rr && pc[d] == cc)
                return fail(TWOSD_E_ARG, "positions %d and %d are the same element (row %d, %s %d)", d, e, row[e],
                            cc < 0 ? "RHS, column" : "column", col[e]);
        pr[e] = rr; pc[e] = cc;
    }
    c->pos_row.swap(pr); c->pos_col.swap(pc);
    c->k = k;
    pool_positions_changed(c);
    c->has_dist = false;
    c->has_blocks = false;
    c->has_lintr = false;
    cut_invalidate_pk(c);
    c->reform = twosd::ReformState();   // stored picks and the re-formation's template copies
    c->fray = twosd::FrayState();   // the feasibility rays and their workspaces
    return TWOSD_OK;
}

// template value at position e (RHS or T entry), in the caller's space: the caller's r, not the
// shifted r' of a template with general bounds (a delta is the same in both)
double twosd::template_value(const twosd_ctx *c, int e) {
    const int rr = c->pos_row[e], cc = c->pos_col[e];
    return cc < 0 ? c->r_user[rr] : c->T[(size_t)rr * c->n1 + cc];
}

// b = r - T x + effect of the element deltas dv (k)
void twosd::rhs_at(const twosd_ctx *c, const double *x, const double *dv, std::vector<double> &b) {
    const int m = c->L.m, n1 = c->n1;
    b.assign(c->r.begin(), c->r.end());
    if (x)
        for (int i = 0; i < m; ++i) {
            double s = 0.0;
            for (int j = 0; j < n1; ++j) s += c->T[(size_t)i * n1 + j] * x[j];
            b[i] -= s;
        }
    if (dv)
        for (int e = 0; e < c->k; ++e) {
            const int cc = c->pos_col[e];
            b[c->pos_row[e]] += cc < 0 ? dv[e] : -dv[e] * (x ? x[cc] : 0.0);
        }
}

extern "C" int twosd_epigraph_create(twosd_ctx *c, int *epi_out) {
    if (!c || !c->has_template || !epi_out) return fail(TWOSD_E_STATE, "epigraph_create: no template");
    c->epis.emplace_back();
    *epi_out = (int)c->epis.size() - 1;
    return TWOSD_OK;
}

extern "C" int twosd_add_scenarios(twosd_ctx *c, int epi, int N, const double *values, const double *weights) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "add_scenarios: no template");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "add_scenarios: epigraph %d does not exist", epi);
    if (N < 0 || (N > 0 && c->k > 0 && !values)) return fail(TWOSD_E_ARG, "add_scenarios: bad arguments");
    if (N == 0) return TWOSD_OK;
    HIPCHK(hipSetDevice(c->device));
    EpiDevice &E = c->epis[epi];
    const int k = c->k;
    std::vector<double> dv((size_t)N * k), w(N, 1.0);
    for (int s = 0; s < N; ++s)
        for (int e = 0; e < k; ++e) dv[(size_t)s * k + e] = values[(size_t)s * k + e] - template_value(c, e);
    if (weights)
        for (int s = 0; s < N; ++s) {
            if (!(weights[s] >= 0.0) || !std::isfinite(weights[s])) return fail(TWOSD_E_ARG, "weight[%d] = %g must be finite and >= 0", s, weights[s]);
            w[s] = weights[s];
        }
    int rc;
    if ((rc = E.d_dv.grow((size_t)(E.count + N) * k, (size_t)E.count * k, c->stream))) return rc;
    if ((rc = E.d_w.grow((size_t)(E.count + N), (size_t)E.count, c->stream))) return rc;
    if (k) HIPCHK(hipMemcpy(E.d_dv + (size_t)E.count * k, dv.data(), sizeof(double) * N * k, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(E.d_w + E.count, w.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    E.w_host.insert(E.w_host.end(), w.begin(), w.end());
    for (int s = 0; s < N; ++s) E.total_weight += w[s];   // epigraph.jl:89, in insertion order
    E.count += N;
    return TWOSD_OK;
}

// twosd_set_distributions (nblocks == 0, kind 3 unknown), twosd_set_distributions_joint and
// twosd_set_distributions_lintr (lintr with blocks: kind 4 known): every check runs before the
// first upload, so a refused call leaves the previous tables in use
static int set_distributions(twosd_ctx *c, int k, const int *kind, const int *nsupport, const double *values, const double *probs,
                             const double *param0, const double *param1, bool joint, int nblocks, const int *member_off,
                             const int *members, const int *nreal, const double *block_probs, const double *block_values,
                             const twosd_lintr *lintr = nullptr) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "set_distributions: no template");
    if (k != c->k) return fail(TWOSD_E_ARG, "set_distributions: %d distributions for %d random elements", k, c->k);
    if (k > 0 && (!kind || !nsupport || !param0 || !param1)) return fail(TWOSD_E_ARG, "set_distributions: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int> kd(std::max(k, 1), 0), off(k + 1, 0);
    std::vector<double> val, prob, p0(std::max(k, 1), 0.0), p1(std::max(k, 1), 0.0), tmpl(std::max(k, 1), 0.0);
    size_t at = 0;
    for (int e = 0; e < k; ++e) {
        kd[e] = kind[e];
        tmpl[e] = template_value(c, e);
        if (kind[e] == 0) {   // DISCRETE: DiscreteNonParametric sorts its support, values unique
            const int n = nsupport[e];
            if (n < 1 || !values || !probs) return fail(TWOSD_E_ARG, "set_distributions: element %d has an empty support", e);
            std::vector<std::pair<double, double>> sp(n);
            for (int i = 0; i < n; ++i) sp[i] = {values[at + i], probs[at + i]};
            at += n;
            std::stable_sort(sp.begin(), sp.end(), [](const std::pair<double, double> &a, const std::pair<double, double> &b) { return a.first < b.first; });
            for (int i = 0; i < n; ++i) {
                if (i && sp[i].first == sp[i - 1].first) return fail(TWOSD_E_ARG, "set_distributions: element %d support values not unique", e);
                if (!(sp[i].second >= 0.0)) return fail(TWOSD_E_ARG, "set_distributions: element %d has a negative probability", e);
                val.push_back(sp[i].first);
                prob.push_back(sp[i].second);
            }
        } else if (kind[e] == 1) {   // NORMAL(mean, variance) -> Normal(mean, sqrt(variance)), smps_sto.jl:122-125
            if (!(param1[e] >= 0.0)) return fail(TWOSD_E_ARG, "set_distributions: element %d has a negative variance", e);
            p0[e] = param0[e];
            p1[e] = std::sqrt(param1[e]);
        } else if (kind[e] == 2) {   // UNIFORM(left, right)
            p0[e] = param0[e];
            p1[e] = param1[e];
        } else if (!(joint && kind[e] == TWOSD_DIST_BLOCK) && !(lintr && kind[e] == TWOSD_DIST_LINTR)) {   // a member's values come from its block
            return fail(TWOSD_E_ARG, "set_distributions: element %d has unknown kind %d", e, kind[e]);
        }
        off[e + 1] = (int)val.size();
    }
    DistTables B;
    int where = -1;
    if (const int err = dist_tables_build(k, kind, joint ? nblocks : 0, member_off, members, nreal, block_probs, block_values, B, &where)) {
        return fail(err == DT_E_TOO_LARGE ? TWOSD_E_UNSUPPORTED : TWOSD_E_ARG, "set_distributions_joint: %s (%s %d)", dist_err_text(err),
                    err == DT_E_NO_BLOCK ? "element" : "block", where);
    }
    LintrTables LT;
    if (lintr) {
        const LintrSpec spec{lintr->nblocks, lintr->member_off, lintr->members, lintr->constants, lintr->latent_off,
                             lintr->latent_kind, lintr->latent_nsupport, lintr->latent_values, lintr->latent_probs,
                             lintr->latent_param0, lintr->latent_param1, lintr->row_ptr, lintr->col, lintr->val};
        if (const int err = lintr_tables_build(k, kind, spec, LT, &where))
            return fail(err == LT_E_TOO_LARGE ? TWOSD_E_UNSUPPORTED : TWOSD_E_ARG, "set_distributions_lintr: %s (%s %d)", lintr_err_text(err),
                        err == LT_E_NO_BLOCK ? "element" : err >= LT_E_LATENT_KIND ? "latent" : "LINTR block", where);
    }
    int rc;
    if ((rc = c->d_dist_kind.upload(kd)) || (rc = c->d_dist_off.upload(off)) || (rc = c->d_dist_val.upload(val)) ||
        (rc = c->d_dist_prob.upload(prob)) || (rc = c->d_dist_p0.upload(p0)) || (rc = c->d_dist_p1.upload(p1)) ||
        (rc = c->d_dist_tmpl.upload(tmpl)))
        return rc;
    c->has_blocks = false;
    if (B.block.empty()) {   // a plain call, or a joint one without blocks, drops the block tables
        c->d_dist_elead.release(); c->d_dist_eblk.release(); c->d_dist_ecol.release();
        c->d_dist_binfo.release(); c->d_dist_bcum.release(); c->d_dist_bval.release();
    } else if ((rc = c->d_dist_elead.upload(B.lead)) || (rc = c->d_dist_eblk.upload(B.blk)) || (rc = c->d_dist_ecol.upload(B.col)) ||
               (rc = c->d_dist_binfo.upload(B.block)) || (rc = c->d_dist_bcum.upload(B.cum)) || (rc = c->d_dist_bval.upload(B.val))) {
        c->has_dist = false;   // a failed upload leaves no usable tables
        return rc;
    }
    if ((rc = upload_lintr(c, LT))) {   // without LINTR blocks: drops their tables
        c->has_dist = false;
        return rc;
    }
    // mean absolute deviation E|V_e - E V_e| per element: the spread of the scenarios (the scale
    // of the selection key's count weight)
    c->dist_mad.assign(std::max(k, 1), 0.0);
    for (int e = 0; e < k; ++e) {
        double mad = 0.0;
        if (kd[e] == 0) {
            double ps = 0.0, mu = 0.0;
            for (int i = off[e]; i < off[e + 1]; ++i) { mu += prob[i] * val[i]; ps += prob[i]; }
            mu = ps > 0.0 ? mu / ps : 0.0;
            for (int i = off[e]; i < off[e + 1]; ++i) mad += prob[i] * fabs(val[i] - mu);
            mad = ps > 0.0 ? mad / ps : 0.0;
        } else if (kd[e] == 1) {   // Normal(mu, sigma): sigma sqrt(2 / pi)
            mad = p1[e] * std::sqrt(2.0 / M_PI);
        } else if (kd[e] == TWOSD_DIST_BLOCK) {   // the member's marginal over the realisations
            mad = dist_member_mad(B, B.blk[e], B.col[e]);
        } else if (kd[e] == TWOSD_DIST_LINTR) {   // the normal-scale heuristic of lintr_tables.h
            mad = lintr_member_mad(LT, LT.row[e]);
        } else {                   // Uniform(a, b): |b - a| / 4
            mad = 0.25 * fabs(p1[e] - p0[e]);
        }
        c->dist_mad[e] = std::isfinite(mad) ? mad : 0.0;
    }
    c->has_blocks = !B.block.empty();
    c->has_dist = true;
    return TWOSD_OK;
}

extern "C" int twosd_set_distributions(twosd_ctx *c, int k, const int *kind, const int *nsupport, const double *values,
                                       const double *probs, const double *param0, const double *param1) {
    return set_distributions(c, k, kind, nsupport, values, probs, param0, param1, false, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int twosd_set_distributions_joint(twosd_ctx *c, int k, const int *kind, const int *nsupport, const double *values,
                                             const double *probs, const double *param0, const double *param1, int nblocks,
                                             const int *member_off, const int *members, const int *nreal,
                                             const double *block_probs, const double *block_values) {
    if (nblocks < 0) return fail(TWOSD_E_ARG, "set_distributions_joint: nblocks < 0");
    return set_distributions(c, k, kind, nsupport, values, probs, param0, param1, true, nblocks, member_off, members, nreal,
                             block_probs, block_values);
}

extern "C" int twosd_set_distributions_lintr(twosd_ctx *c, int k, const int *kind, const int *nsupport, const double *values,
                                             const double *probs, const double *param0, const double *param1, int nblocks,
                                             const int *member_off, const int *members, const int *nreal,
                                             const double *block_probs, const double *block_values, const twosd_lintr *lintr) {
    if (nblocks < 0) return fail(TWOSD_E_ARG, "set_distributions_lintr: nblocks < 0");
    if (lintr && lintr->nblocks < 0) return fail(TWOSD_E_ARG, "set_distributions_lintr: lintr->nblocks < 0");
    return set_distributions(c, k, kind, nsupport, values, probs, param0, param1, true, nblocks, member_off, members, nreal,
                             block_probs, block_values, lintr && lintr->nblocks > 0 ? lintr : nullptr);
}

// a caller's sampling plan -> (mode, G); NULL means i.i.d.
int twosd::sampling_plan(const twosd_sampling *plan, const char *who, int *mode, int *G) {
    *mode = TWOSD_SAMPLING_IID;
    *G = 1;
    if (!plan) return TWOSD_OK;
    switch (plan->mode) {
    case TWOSD_SAMPLING_IID:
        if (plan->group != 1) return fail(TWOSD_E_ARG, "%s: an IID plan has group 1, not %d", who, plan->group);
        break;
    case TWOSD_SAMPLING_ANTITHETIC:
        if (plan->group != 2) return fail(TWOSD_E_ARG, "%s: an ANTITHETIC plan has group 2, not %d", who, plan->group);
        break;
    case TWOSD_SAMPLING_LHS:
        if (plan->group < 2 || plan->group > 256)
            return fail(TWOSD_E_ARG, "%s: an LHS plan needs 2 <= group <= 256, not %d", who, plan->group);
        break;
    default:
        return fail(TWOSD_E_ARG, "%s: unknown sampling mode %d", who, plan->mode);
    }
    *mode = plan->mode;
    *G = plan->group;
    return TWOSD_OK;
}

// `what` = value must be a whole number of groups
int twosd::whole_groups(const char *who, const char *what, unsigned long long value, int G) {
    if (G > 1 && value % (unsigned long long)G)
        return fail(TWOSD_E_ARG, "%s: %s = %llu is no multiple of the sampling group %d", who, what, value, G);
    return TWOSD_OK;
}

SampleParams twosd::sample_params(const twosd_ctx *c, int n, uint64_t seed, uint64_t first_index, double *out) {
    SampleParams S{};
    S.N = n; S.k = c->k; S.seed = seed; S.first_index = first_index;
    S.kind = c->d_dist_kind; S.off = c->d_dist_off; S.val = c->d_dist_val; S.prob = c->d_dist_prob;
    S.p0 = c->d_dist_p0; S.p1 = c->d_dist_p1; S.tmpl = c->d_dist_tmpl; S.out = out;
    S.blocks = c->has_blocks;
    S.elead = c->d_dist_elead; S.eblk = c->d_dist_eblk; S.ecol = c->d_dist_ecol;
    S.binfo = c->d_dist_binfo; S.bcum = c->d_dist_bcum; S.bval = c->d_dist_bval;
    return S;
}

static int add_sampled(twosd_ctx *c, int epi, int N, uint64_t seed, uint64_t first_index, const double *weights, int mode,
                       int G);

extern "C" int twosd_add_sampled_scenarios(twosd_ctx *c, int epi, int N, uint64_t seed, uint64_t first_index,
                                           const double *weights) {
    return add_sampled(c, epi, N, seed, first_index, weights, TWOSD_SAMPLING_IID, 1);
}

extern "C" int twosd_add_sampled_scenarios_vr(twosd_ctx *c, int epi, int N, uint64_t seed, uint64_t first_index,
                                              const double *weights, const twosd_sampling *plan) {
    int mode, G, rc;
    if ((rc = sampling_plan(plan, "add_sampled_scenarios", &mode, &G))) return rc;
    if (N > 0 && ((rc = whole_groups("add_sampled_scenarios", "first_index", first_index, G)) ||
                  (rc = whole_groups("add_sampled_scenarios", "N", (unsigned long long)N, G))))
        return rc;
    return add_sampled(c, epi, N, seed, first_index, weights, mode, G);
}

static int add_sampled(twosd_ctx *c, int epi, int N, uint64_t seed, uint64_t first_index, const double *weights, int mode,
                       int G) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "add_sampled_scenarios: no template");
    if (!c->has_dist) return fail(TWOSD_E_STATE, "add_sampled_scenarios: no distributions (twosd_set_distributions)");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "add_sampled_scenarios: epigraph %d does not exist", epi);
    if (N < 0) return fail(TWOSD_E_ARG, "add_sampled_scenarios: N < 0");
    if (N == 0) return TWOSD_OK;
    HIPCHK(hipSetDevice(c->device));
    EpiDevice &E = c->epis[epi];
    const int k = c->k;
    std::vector<double> w(N, 1.0);
    if (weights)
        for (int s = 0; s < N; ++s) {
            if (!(weights[s] >= 0.0) || !std::isfinite(weights[s])) return fail(TWOSD_E_ARG, "weight[%d] = %g must be finite and >= 0", s, weights[s]);
            w[s] = weights[s];
        }
    int rc;
    if ((rc = E.d_dv.grow((size_t)(E.count + N) * k, (size_t)E.count * k, c->stream))) return rc;
    if ((rc = E.d_w.grow((size_t)(E.count + N), (size_t)E.count, c->stream))) return rc;
    if ((rc = draw_scenarios(c, N, seed, first_index, E.d_dv + (size_t)E.count * k, mode, G))) return rc;
    HIPCHK(hipMemcpyAsync(E.d_w + E.count, w.data(), sizeof(double) * N, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    E.w_host.insert(E.w_host.end(), w.begin(), w.end());
    for (int s = 0; s < N; ++s) E.total_weight += w[s];   // epigraph.jl:89, in insertion order
    E.count += N;
    return TWOSD_OK;
}

extern "C" int twosd_get_scenarios(twosd_ctx *c, int epi, int first, int count, double *values) {
    if (!c || epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "get_scenarios: bad epigraph");
    const EpiDevice &E = c->epis[epi];
    if (first < 0 || count < 0 || first + count > E.count || (count > 0 && c->k > 0 && !values))
        return fail(TWOSD_E_ARG, "get_scenarios: range [%d,%d) outside %d scenarios", first, first + count, E.count);
    if (count == 0 || c->k == 0) return TWOSD_OK;
    HIPCHK(hipSetDevice(c->device));
    const int k = c->k;
    HIPCHK(hipMemcpy(values, E.d_dv + (size_t)first * k, sizeof(double) * count * k, hipMemcpyDeviceToHost));
    for (int s = 0; s < count; ++s)
        for (int e = 0; e < k; ++e) values[(size_t)s * k + e] += template_value(c, e);
    return TWOSD_OK;
}

extern "C" int twosd_epigraph_info(twosd_ctx *c, int epi, int *ns, double *tw) {
    if (!c || epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "epigraph_info: bad epigraph");
    if (ns) *ns = c->epis[epi].count;
    if (tw) *tw = c->epis[epi].total_weight;
    return TWOSD_OK;
}
