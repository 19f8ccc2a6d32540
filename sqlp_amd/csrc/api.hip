// api.hip -- C ABI of libtwosd_hip.so (declared in include/twosd_hip.h).
//
// Owns the device-resident state of the TwoSD hot path on one MI355X:
//   template (W CSC, q, bound types), shared warm-start basis (B0^{-1}, pi0), per-epigraph
//   scenario pools (deltas, weights), the dual vertex set, and the LP/cut workspaces.
// Every call is synchronous on the context's own HIP stream.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <map>
#include <memory>
#include <thread>
#include <chrono>
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
    for (int i = 0; i < 8; ++i) HIPCHK(hipEventCreate(&c->ev[i]));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    c->num_cus = prop.multiProcessorCount;
    const char *km = getenv("TWOSD_KMAX");
    if (km) c->kmax_override = atoi(km);
    *out = c.release();
    return TWOSD_OK;
}

// Sliced ELL of S*64 columns: column j = 64*s + l gives (row, value) entries via colf.
// Slot s has width E_s = max entries over its 64 columns; entry e of lane l is stored at
// [(slot[s] + e) * 64 + l], padding (row 0, value 0).
template <typename F>
static void build_ell(int S, F colf, std::vector<int> &slot, std::vector<int> &ix, std::vector<double> &v) {
    slot.assign(S + 1, 0);
    std::vector<std::vector<std::pair<int, double>>> cols(64);
    ix.clear(); v.clear();
    for (int s = 0; s < S; ++s) {
        int width = 0;
        for (int l = 0; l < 64; ++l) {
            cols[l].clear();
            colf(64 * s + l, cols[l]);
            width = std::max(width, (int)cols[l].size());
        }
        for (int e = 0; e < width; ++e)
            for (int l = 0; l < 64; ++l) {
                const bool has = e < (int)cols[l].size();
                ix.push_back(has ? cols[l][e].first : 0);
                v.push_back(has ? cols[l][e].second : 0.0);
            }
        slot[s + 1] = slot[s] + width;
    }
}

// the two-level candidate lists (device, or staged for the next selection) refer to pool
// indices: every change of the pool drops them
void twosd::reset_candidates(twosd_ctx *c) {
    c->pool_l1 = c->pool_ncand = 0;
    c->cand_pending = false;
    std::vector<int>().swap(c->cand_p1);
    std::vector<int>().swap(c->cand_pf);
}

// the pool no longer matches the device arrays (a failed build or head read-back): keep only
// the primary basis (a host basis) and refuse solves until a basis is installed again
int twosd::drop_pool(twosd_ctx *c, int code) {
    if (c->pool.size() > 1) c->pool.resize(1);
    c->has_basis = false;
    c->prep_valid = false;
    c->k_valid = false;
    c->pool_hb_valid = false;
    reset_candidates(c);
    return code;
}

// head of pool basis p into *h (materialised from c->pool_hb for a device-built basis on first
// use: a refresh of 4096 bases would otherwise spend ~2 ms building host heads nobody reads).
// A failed device read-back drops the pool (drop_pool) and returns TWOSD_E_DEVICE.
static int head_of(twosd_ctx *c, int p, const std::vector<int> **h) {
    PoolBasis &B = c->pool[p];
    if (B.hb_row >= 0 && !c->pool_hb_valid) {
        // the heads of a device-built pool are fetched on the first host use, not by the refresh
        // (at N = 8 every rank would copy 9 MB per step that only tests and the CPU baseline read)
        const size_t need = c->pool.size() * (size_t)c->MP;
        if (!c->pool_hb.reserve<int>(need))
            return drop_pool(c, fail(TWOSD_E_DEVICE, "pool heads: pinned allocation of %zu ints failed", need));
        hipError_t e = hipMemcpyAsync(c->pool_hb.p, c->d_hb0, sizeof(int) * need, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return drop_pool(c, fail(TWOSD_E_DEVICE, "pool heads: read-back failed: %s", hipGetErrorString(e)));
        c->pool_hb_valid = true;
    }
    if (B.hb_row >= 0) {
        const int m = c->L.m;
        const int *r = c->pool_hb.as<int>() + (size_t)B.hb_row * c->MP;
        B.head.resize(m);
        for (int i = 0; i < m; ++i) B.head[i] = r[i] >> 2;
        B.hb_row = -1;
    }
    if (h) *h = &B.head;
    return TWOSD_OK;
}
static int materialize_heads(twosd_ctx *c) {
    for (int p = 0; p < (int)c->pool.size(); ++p)
        if (int rc = head_of(c, p, nullptr)) return rc;
    return TWOSD_OK;
}

// device selection-stream outputs of a pool of P bases with `records` records (prepare_x
// writes them per x)
int twosd::reserve_selection(twosd_ctx *c, int P, int records) {
    int rc;
    if ((rc = c->d_sel_code.fit(2 * (size_t)std::max(records, 1)))) return rc;   // (code, float bits) pairs
    if ((rc = c->d_sel_end.reserve((size_t)P)) || (rc = c->d_sel_cinf.reserve((size_t)P))) return rc;
    c->sel_cap_total = records;
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
    c->prep_valid = false;
    c->k_valid = false;
    c->has_dist = false;
    cut_invalidate_pk(c);
    c->boot = twosd::BootState();   // stored picks and the re-formation's template copies
    return TWOSD_OK;
}

// template value at position e (RHS or T entry), in the caller's space: the caller's r, not the
// shifted r' of a template with general bounds (a delta is the same in both)
static double template_value(const twosd_ctx *c, int e) {
    const int rr = c->pos_row[e], cc = c->pos_col[e];
    return cc < 0 ? c->r_user[rr] : c->T[(size_t)rr * c->n1 + cc];
}

// b = r - T x + effect of the element deltas dv (k)
static void rhs_at(const twosd_ctx *c, const double *x, const double *dv, std::vector<double> &b) {
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
int twosd::ensure_host_pool(twosd_ctx *c) {
    if (int rc = materialize_heads(c)) return rc;
    const int P = (int)c->pool.size(), MP = c->MP, m = c->L.m;
    int last = -1;
    for (int p = 0; p < P; ++p)
        if (c->pool[p].dev_only) last = p;
    if (last < 0) return TWOSD_OK;
    const int Pd = last + 1;
    std::vector<int> rp((size_t)Pd * (MP + 1));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(rp.data(), c->d_brptr, sizeof(int) * rp.size(), hipMemcpyDeviceToHost));
    size_t nz = 0;
    for (int p = 0; p < Pd; ++p) nz = std::max(nz, (size_t)rp[(size_t)p * (MP + 1) + m]);
    std::vector<int> col(std::max<size_t>(nz, 1));
    std::vector<double> val(std::max<size_t>(nz, 1));
    if (nz) {
        HIPCHK(hipMemcpy(col.data(), c->d_brcol, sizeof(int) * nz, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(val.data(), c->d_brval, sizeof(double) * nz, hipMemcpyDeviceToHost));
    }
    parallel_for(Pd, [&](int p) {
        PoolBasis &B = c->pool[p];
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

// Upload the hypersparse-kernel form of every pool basis, pool-strided (pool[0] first, so
// the leading MP / 64 / 64C entries are the primary basis): hb0 (MP), basic0 (64),
// d0 (64C), B^{-1} columns as CSC (bcp absolute into the concatenated bci/bcv),
// B^{-1} rows as CSR (brptr absolute into the concatenated brcol/brval).
int twosd::upload_pool(twosd_ctx *c) {
    const auto t_up0 = std::chrono::steady_clock::now();
    if (int rc0 = ensure_host_pool(c)) return rc0;
    const HostLP &L = c->L;
    const int m = L.m, n = L.n, MP = c->MP, P = (int)c->pool.size();
    std::vector<int8_t> bt(n + m);
    HIPCHK(hipMemcpy(bt.data(), c->d_btype, n + m, hipMemcpyDeviceToHost));
    std::vector<int> hb((size_t)P * MP, -1), bnnz(P, 0);
    std::vector<uint64_t> basic((size_t)P * 64, 0);
    // B^{-1} of every basis by rows (CSR) and by columns (CSC, rows ascending), both at the same
    // per-basis offset ro[p]; offsets are known up front, so every basis fills its part of the
    // concatenated arrays directly (default-initialised buffers, first touch in parallel)
    std::vector<size_t> ro(P + 1, 0);
    for (int p = 0; p < P; ++p) ro[p + 1] = ro[p] + c->pool[p].rcol.size();
    if (ro[P] > INT32_MAX) return fail(TWOSD_E_UNSUPPORTED, "basis pool too large (> 2^31 entries)");
    const size_t nz = std::max<size_t>(ro[P], 1);
    std::vector<int> rp_all((size_t)P * (MP + 1)), cp_all((size_t)P * (MP + 1));
    int *rc_all = c->stage[STG_POOL_RCOL].reserve<int>(nz), *ci_all = c->stage[STG_POOL_CROW].reserve<int>(nz);
    double *rv_all = c->stage[STG_POOL_RVAL].reserve<double>(nz), *cv_all = c->stage[STG_POOL_CVAL].reserve<double>(nz);
    double *d0_all = c->stage[STG_POOL_D0].reserve<double>((size_t)P * 64 * std::max(c->CH, 1));
    if (!rc_all || !ci_all || !rv_all || !cv_all || !d0_all) return fail(TWOSD_E_DEVICE, "pool upload: pinned staging allocation failed");
    parallel_for(P, [&](int p) {
        const PoolBasis &B = c->pool[p];
        std::vector<char> isb(n + m, 0);
        for (int i = 0; i < m; ++i) {
            hb[(size_t)p * MP + i] = B.head[i] * 4 + bt[B.head[i]];
            basic[(size_t)p * 64 + (B.head[i] & 63)] |= 1ull << (B.head[i] >> 6);
            isb[B.head[i]] = 1;
        }
        bnnz[p] = (int)B.rcol.size();
        const int base = (int)ro[p];
        for (int i = 0; i <= MP; ++i) rp_all[(size_t)p * (MP + 1) + i] = base + B.rptr[std::min(i, m)];
        std::copy(B.rcol.begin(), B.rcol.end(), rc_all + base);
        std::copy(B.rval.begin(), B.rval.end(), rv_all + base);
        // columns: counting sort of the row CSR (rows ascending within a column)
        std::vector<int> pos(m + 1, 0);
        for (int cc : B.rcol) ++pos[cc + 1];
        for (int cc = 0; cc < m; ++cc) pos[cc + 1] += pos[cc];
        for (int cc = 0; cc <= MP; ++cc) cp_all[(size_t)p * (MP + 1) + cc] = base + pos[std::min(cc, m)];
        for (int i = 0; i < m; ++i)
            for (int q = B.rptr[i]; q < B.rptr[i + 1]; ++q) {
                const int at = base + pos[B.rcol[q]]++;
                ci_all[at] = i;
                cv_all[at] = B.rval[q];
            }
        if (c->CH <= 0) return;
        double *d0 = d0_all + (size_t)p * 64 * c->CH;
        for (int j = 0; j < 64 * c->CH; ++j) {
            if (j >= n + m || isb[j]) { d0[j] = 0.0; continue; }
            double sum = 0.0;
            if (j >= n) sum = B.pi0[j - n];
            else
                for (int q = L.colptr[j]; q < L.colptr[j + 1]; ++q) sum += B.pi0[L.rowidx[q]] * L.val[q];
            d0[j] = (j < n ? L.q[j] : 0.0) - sum;
        }
    });
    const auto tc = std::chrono::steady_clock::now();
    int rc;
    if ((rc = c->d_hb0.upload_reserve(hb)) || (rc = c->d_basic0.upload_reserve(basic)) || (rc = c->d_bnnz.upload_reserve(bnnz))) return rc;
    if (c->CH > 0) {
        if ((rc = c->d_bcp.upload_reserve(cp_all)) || (rc = c->d_bci.upload_reserve(ci_all, ro[P])) ||
            (rc = c->d_bcv.upload_reserve(cv_all, ro[P])) || (rc = c->d_brptr.upload_reserve(rp_all)) ||
            (rc = c->d_brcol.upload_reserve(rc_all, ro[P])) || (rc = c->d_brval.upload_reserve(rv_all, ro[P])) ||
            (rc = c->d_d0.upload_reserve(d0_all, (size_t)P * 64 * c->CH)))
            return rc;
        c->b0_nnz = bnnz[0];
    }
    if (getenv("TWOSD_DEBUG")) {
        const auto td = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "upload_pool P=%d: build %.1f ms, upload %.1f ms (%.1f MB, %zu nonzeros)\n", P, ms(t_up0, tc), ms(tc, td),
                (ro[P] * 24.0 + (size_t)P * 64 * std::max(c->CH, 0) * 8.0) / 1e6, ro[P]);
    }
    c->prep_valid = false;
    c->k_valid = false;
    reset_candidates(c);   // candidate lists refer to pool indices: rebuild after a change
    return TWOSD_OK;
}

static int install_basis(twosd_ctx *c, const std::vector<int> &head) {
    PoolBasis pb;
    int rc = make_pool_basis(c, head, pb);
    if (rc) return rc;
    c->head0 = head;
    c->pool.clear();
    c->sel_lo.clear();
    c->sel_hi.clear();
    c->sel_box = BoxCache{};
    c->pool.push_back(std::move(pb));
    if ((rc = upload_pool(c))) return rc;
    c->has_basis = true;
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
    for (const PoolBasis &B : c->pool)
        if (same_basis(B.head, head)) return 0;
    PoolBasis pb;
    int rc = make_pool_basis(c, head, pb);
    if (rc) return rc;
    std::vector<double>().swap(pb.Binv);
    c->pool.push_back(std::move(pb));
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
    if (!c || !c->has_basis || !head) return fail(TWOSD_E_STATE, "get_basis: no basis");
    std::copy(c->head0.begin(), c->head0.end(), head);
    return TWOSD_OK;
}

extern "C" int twosd_pool_add_basis(twosd_ctx *c, const int *head, int *added) {
    if (!c || !c->has_basis || !head) return fail(TWOSD_E_STATE, "pool_add_basis: no primary basis / NULL head");
    HIPCHK(hipSetDevice(c->device));
    const int rc = pool_add(c, std::vector<int>(head, head + c->L.m), true);
    if (rc < 0) return rc;
    if (added) *added = rc;
    return TWOSD_OK;
}

extern "C" int twosd_pool_size(twosd_ctx *c, int *size) {
    if (!c || !size) return fail(TWOSD_E_ARG, "pool_size: NULL argument");
    *size = (int)c->pool.size();
    return TWOSD_OK;
}

extern "C" int twosd_pool_get(twosd_ctx *c, int p, int *head) {
    if (c && !c->has_basis) return fail(TWOSD_E_STATE, "pool_get: no basis");
    if (!c || !head || p < 0 || p >= (int)c->pool.size()) return fail(TWOSD_E_ARG, "pool_get: basis %d of %zu", p, c ? c->pool.size() : 0);
    const std::vector<int> *h = nullptr;
    if (int rc = head_of(c, p, &h)) return rc;
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

int twosd::training_box(twosd_ctx *c, const EpiDevice &E, int epi, int first, int count, std::vector<double> &lo,
                        std::vector<double> &hi, BoxCache *cache) {
    const int k = c->k;
    const BoxCache range{epi, first, count, E.count};
    if (k <= 0 || (cache && *cache == range)) return TWOSD_OK;
    std::vector<double> dv((size_t)count * k);
    HIPCHK(hipMemcpy(dv.data(), E.d_dv + (size_t)first * k, sizeof(double) * dv.size(), hipMemcpyDeviceToHost));
    lo.assign(k, INFINITY);
    hi.assign(k, -INFINITY);
    for (int s = 0; s < count; ++s)
        for (int e = 0; e < k; ++e) {
            lo[e] = std::min(lo[e], dv[(size_t)s * k + e]);
            hi[e] = std::max(hi[e], dv[(size_t)s * k + e]);
        }
    if (cache) *cache = range;
    return TWOSD_OK;
}

// Grow the pool from training scenarios [first, first + count) of epigraph epi at x.  The
// first half harvests: solved from the current pool, its optimal bases are added in order
// of decreasing frequency (ties: first occurrence) up to max_pool bases.  The second half
// validates: the grown pool is kept only if it solves those scenarios in fewer pivots.
extern "C" int twosd_pool_build(twosd_ctx *c, int epi, const double *x, int first, int count, int max_pool,
                                int *pool_size) {
    if (!c || !c->has_basis) return fail(TWOSD_E_STATE, "pool_build: no primary basis");
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
    if (nh > 0 && (int)c->pool.size() < max_pool) {
        const double *dh = E.d_dv + (size_t)first * c->k, *dval = dh + (size_t)nh * c->k;
        int rc;
        if ((rc = run_lp(c, x, dval, nv, false, false))) return rc;
        const int64_t piv0 = pivots_of_last_lp(c, nv);
        c->want_head = true;
        rc = run_lp(c, x, dh, nh, false, false);
        c->want_head = false;
        if (rc) return rc;
        std::vector<int> heads((size_t)nh * m), st(nh);
        HIPCHK(hipMemcpy(heads.data(), c->d_head_out, sizeof(int) * heads.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(st.data(), c->d_status, sizeof(int) * nh, hipMemcpyDeviceToHost));
        std::map<std::vector<int>, std::pair<int, int>> freq;   // sorted head -> (count, first scenario)
        if ((rc = materialize_heads(c))) return rc;
        for (const PoolBasis &B : c->pool) {
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
        const size_t old_size = c->pool.size();
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
            if (ok[a]) c->pool.push_back(std::move(cand[a]));
        if (c->pool.size() > old_size) {
            if ((rc = upload_pool(c))) return rc;
            if ((rc = run_lp(c, x, dval, nv, false, false))) return rc;
            const int64_t piv1 = pivots_of_last_lp(c, nv);
            std::vector<int> st2(nv);
            HIPCHK(hipMemcpy(st2.data(), c->d_status, sizeof(int) * nv, hipMemcpyDeviceToHost));
            const bool all_ok = std::all_of(st2.begin(), st2.end(), [](int v) { return v == TWOSD_LP_OPTIMAL; });
            if (piv1 < 0 || piv0 < 0 || piv1 >= piv0 || !all_ok) {   // no gain: back to the old pool
                c->pool.resize(old_size);
                if ((rc = upload_pool(c))) return rc;
            }
        }
    }
    if (pool_size) *pool_size = (int)c->pool.size();
    return TWOSD_OK;
}

static int select_pool(twosd_ctx *c, const double *d_dv, int N, int *d_pick, int npool_override);

// Two-level selection from training scenarios [first, first + count) of epigraph epi at x:
// level 1 = pool[0, level1) (the most frequent bases); the candidates of a level-1 basis p are
// the ncand bases that the flat selection over the whole pool picks most often for training
// scenarios whose level-1 pick is p (ties: lower index).  level1 = 0 back to flat selection.
// flat and level-1 picks of training scenarios [first, first + count) of epi at x
static int candidate_picks(twosd_ctx *c, const EpiDevice &E, const double *x, int first, int count, int level1,
                           int *p1, int *pf) {
    int rc;
    if ((rc = prepare_x(c, x))) return rc;
    if ((rc = c->d_cpick.reserve((size_t)count))) return rc;   // grow-only: no reallocation per refresh
    int *d_p = c->d_cpick;
    const double *dv = E.d_dv + (size_t)first * c->k;
    auto picks = [&](int np, int *out) {   // selection runs on c->stream
        int r = select_pool(c, dv, count, d_p, np);
        if (!r && (hipStreamSynchronize(c->stream) != hipSuccess ||
                   hipMemcpy(out, d_p, sizeof(int) * count, hipMemcpyDeviceToHost) != hipSuccess))
            r = fail(TWOSD_E_DEVICE, "pool candidates: selection failed");
        return r;
    };
    rc = picks(level1, p1);
    if (!rc) rc = picks((int)c->pool.size(), pf);
    return rc;
}

// candidate lists from the picks of the training scenarios (any order): the ncand bases the flat
// selection picks most often among the scenarios of each level-1 pick (ties: lower index)
static int set_candidates(twosd_ctx *c, int level1, int ncand, int n, const int *p1, const int *pf) {
    // the differing (level-1 pick, flat pick) pairs bucketed by level-1 pick (counting sort), then
    // per bucket the flat picks sorted and counted by runs; the ncand most frequent kept (ties:
    // lower basis)
    std::vector<int> start(level1 + 1, 0);
    for (int s = 0; s < n; ++s)
        if (pf[s] != p1[s] && p1[s] >= 0 && p1[s] < level1) ++start[p1[s] + 1];
    for (int p = 0; p < level1; ++p) start[p + 1] += start[p];
    std::vector<int> fill(start.begin(), start.end() - 1), bucket(start[level1]);
    for (int s = 0; s < n; ++s)
        if (pf[s] != p1[s] && p1[s] >= 0 && p1[s] < level1) bucket[fill[p1[s]]++] = pf[s];
    std::vector<int> cand((size_t)level1 * ncand, -1);
    std::vector<std::pair<int, int>> v;   // (-count, basis) of one level-1 pick
    for (int p = 0; p < level1; ++p) {
        int *b0 = bucket.data() + start[p], *b1 = bucket.data() + start[p + 1];
        if (b0 == b1) continue;
        std::sort(b0, b1);
        v.clear();
        for (int *a = b0; a < b1;) {
            int *b = a;
            while (b < b1 && *b == *a) ++b;
            v.push_back({-(int)(b - a), *a});
            a = b;
        }
        const size_t nk = std::min<size_t>(v.size(), ncand);
        std::partial_sort(v.begin(), v.begin() + nk, v.end());
        for (size_t i = 0; i < nk; ++i) cand[(size_t)p * ncand + i] = v[i].second;
    }
    if (getenv("TWOSD_DEBUG")) {
        int diff = 0, filled = 0;
        for (int s = 0; s < n; ++s) diff += pf[s] != p1[s];
        for (int v : cand) filled += v >= 0;
        fprintf(stderr, "pool candidates: P=%zu level1=%d: %d of %d training picks change, %d candidate slots filled\n",
                c->pool.size(), level1, diff, n, filled);
    }
    int rc;
    int *h = c->stage[STG_CAND].reserve<int>(cand.size());
    if (!h) return fail(TWOSD_E_DEVICE, "pool candidates: pinned staging allocation failed");
    std::copy(cand.begin(), cand.end(), h);
    if ((rc = c->d_cand.reserve(cand.size()))) return rc;
    HIPCHK(hipMemcpyAsync(c->d_cand, h, sizeof(int) * cand.size(), hipMemcpyHostToDevice, c->stream));
    c->pool_l1 = level1;
    c->pool_ncand = ncand;
    c->cand_pending = false;
    return TWOSD_OK;
}

// the lists are built by the next two-level selection (select_pool), on the host while its
// level-1 pass runs on the device: same lists, the host time off the critical path
static int defer_candidates(twosd_ctx *c, int level1, int ncand, std::vector<int> &&p1, std::vector<int> &&pf) {
    c->cand_p1 = std::move(p1);
    c->cand_pf = std::move(pf);
    c->cand_pl1 = level1;
    c->cand_pnc = ncand;
    c->cand_pending = true;
    c->pool_l1 = level1;
    c->pool_ncand = ncand;
    return TWOSD_OK;
}

extern "C" int twosd_pool_candidate_picks(twosd_ctx *c, int epi, const double *x, int first, int count, int level1, int *p1,
                                          int *pf) {
    if (!c || !c->has_basis) return fail(TWOSD_E_STATE, "pool_candidate_picks: no primary basis");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "pool_candidate_picks: epigraph %d does not exist", epi);
    const EpiDevice &E = c->epis[epi];
    const int P = (int)c->pool.size();
    if (first < 0 || count < 1 || first + count > E.count || level1 < 1 || level1 >= P || !p1 || !pf || (c->n1 > 0 && !x) ||
        c->CH <= 0)
        return fail(TWOSD_E_ARG, "pool_candidate_picks: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    reset_candidates(c);   // the flat pick runs over the whole pool
    return candidate_picks(c, E, x, first, count, level1, p1, pf);
}

extern "C" int twosd_pool_set_candidates(twosd_ctx *c, int level1, int ncand, int n, const int *p1, const int *pf) {
    if (!c || !c->has_basis) return fail(TWOSD_E_STATE, "pool_set_candidates: no primary basis");
    const int P = (int)c->pool.size();
    if (level1 < 1 || level1 >= P || ncand < 1 || ncand > 1024 || n < 0 || (n > 0 && (!p1 || !pf)))
        return fail(TWOSD_E_ARG, "pool_set_candidates: bad arguments");
    for (int s = 0; s < n; ++s)
        if (p1[s] < 0 || p1[s] >= P || pf[s] < 0 || pf[s] >= P) return fail(TWOSD_E_ARG, "pool_set_candidates: pick outside the pool");
    HIPCHK(hipSetDevice(c->device));
    return defer_candidates(c, level1, ncand, std::vector<int>(p1, p1 + n), std::vector<int>(pf, pf + n));
}

extern "C" int twosd_pool_build_candidates(twosd_ctx *c, int epi, const double *x, int first, int count, int level1,
                                           int ncand) {
    if (!c || !c->has_basis) return fail(TWOSD_E_STATE, "pool_build_candidates: no primary basis");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "pool_build_candidates: epigraph %d does not exist", epi);
    const EpiDevice &E = c->epis[epi];
    const int P = (int)c->pool.size();
    if (first < 0 || count < 1 || first + count > E.count || level1 < 0 || ncand < 0 || ncand > 1024 || (c->n1 > 0 && !x))
        return fail(TWOSD_E_ARG, "pool_build_candidates: bad arguments");
    reset_candidates(c);
    if (level1 == 0 || ncand == 0 || level1 >= P || P < 2 || c->CH <= 0) return TWOSD_OK;   // flat selection
    HIPCHK(hipSetDevice(c->device));
    std::vector<int> p1(count), pf(count);
    int rc;
    if ((rc = candidate_picks(c, E, x, first, count, level1, p1.data(), pf.data()))) return rc;
    return defer_candidates(c, level1, ncand, std::move(p1), std::move(pf));
}

extern "C" int twosd_last_pool_picks(twosd_ctx *c, int N, int *picks) {
    if (!c || !picks || N < 0 || N > c->last_lp_N) return fail(TWOSD_E_ARG, "last_pool_picks: bad arguments");
    if (c->pool.size() <= 1 || !c->d_pool_pick) {
        std::fill(picks, picks + N, 0);
        return TWOSD_OK;
    }
    HIPCHK(hipMemcpy(picks, c->d_pool_pick, sizeof(int) * N, hipMemcpyDeviceToHost));
    return TWOSD_OK;
}

extern "C" int twosd_invalidate_x(twosd_ctx *c) {
    if (!c) return fail(TWOSD_E_ARG, "invalidate_x: NULL context");
    c->prep_valid = false;   // (the cut's PK rows do not depend on x: kept)
    return TWOSD_OK;
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

extern "C" int twosd_set_distributions(twosd_ctx *c, int k, const int *kind, const int *nsupport, const double *values,
                                       const double *probs, const double *param0, const double *param1) {
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
        } else {
            return fail(TWOSD_E_ARG, "set_distributions: element %d has unknown kind %d", e, kind[e]);
        }
        off[e + 1] = (int)val.size();
    }
    int rc;
    if ((rc = c->d_dist_kind.upload(kd)) || (rc = c->d_dist_off.upload(off)) || (rc = c->d_dist_val.upload(val)) ||
        (rc = c->d_dist_prob.upload(prob)) || (rc = c->d_dist_p0.upload(p0)) || (rc = c->d_dist_p1.upload(p1)) ||
        (rc = c->d_dist_tmpl.upload(tmpl)))
        return rc;
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
        } else {                   // Uniform(a, b): |b - a| / 4
            mad = 0.25 * fabs(p1[e] - p0[e]);
        }
        c->dist_mad[e] = std::isfinite(mad) ? mad : 0.0;
    }
    c->has_dist = true;
    return TWOSD_OK;
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
    SampleParams S{};
    S.N = N; S.k = k; S.seed = seed; S.first_index = first_index;
    S.kind = c->d_dist_kind; S.off = c->d_dist_off; S.val = c->d_dist_val; S.prob = c->d_dist_prob;
    S.p0 = c->d_dist_p0; S.p1 = c->d_dist_p1; S.tmpl = c->d_dist_tmpl; S.out = E.d_dv + (size_t)E.count * k;
    HIPCHK(launch_sample_plan(S, mode, G, c->stream));
    HIPCHK(hipMemcpyAsync(E.d_w + E.count, w.data(), sizeof(double) * N, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    E.w_host.insert(E.w_host.end(), w.begin(), w.end());
    for (int s = 0; s < N; ++s) E.total_weight += w[s];   // epigraph.jl:89, in insertion order
    E.count += N;
    return TWOSD_OK;
}

static int copy_lp_outputs(twosd_ctx *c, int N, double *obj, double *pi, double *y, int *status, const double *d_w);

// evaluate(sp1, sp2, sto, x; N) stage-2 part (smps_routines.jl:67-82) on device-drawn
// scenarios: *s2 = sum over scenarios first..first+count-1 of the stream `seed`, in index
// order, of (1/N_total) * obj (s2_cost += 1/N*obj, :79).  Chunks of <= 1M scenarios:
// sample into scratch, LP solve (objective only), objectives summed on the host in order.
extern "C" int twosd_evaluate_sampled(twosd_ctx *c, const double *x, int64_t N_total, int64_t first, int64_t count,
                                      uint64_t seed, double *s2) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "evaluate_sampled: no template");
    if (!c->has_basis) return fail(TWOSD_E_STATE, "evaluate_sampled: no warm-start basis");
    if (!c->has_dist) return fail(TWOSD_E_STATE, "evaluate_sampled: no distributions (twosd_set_distributions)");
    if (!s2 || N_total <= 0 || first < 0 || count < 0 || (c->n1 > 0 && !x)) return fail(TWOSD_E_ARG, "evaluate_sampled: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    const int k = c->k;
    const int64_t chunk = 1 << 20;
    const double invN = 1.0 / (double)N_total;
    double acc = 0.0;
    std::vector<double> obj;
    for (int64_t at = 0; at < count; at += chunk) {
        const int n = (int)std::min(chunk, count - at);
        int rc;
        if ((rc = c->d_dvtmp.grow((size_t)n * std::max(k, 1), 0, c->stream))) return rc;
        SampleParams S{};
        S.N = n; S.k = k; S.seed = seed; S.first_index = (unsigned long long)(first + at);
        S.kind = c->d_dist_kind; S.off = c->d_dist_off; S.val = c->d_dist_val; S.prob = c->d_dist_prob;
        S.p0 = c->d_dist_p0; S.p1 = c->d_dist_p1; S.tmpl = c->d_dist_tmpl; S.out = c->d_dvtmp;
        HIPCHK(launch_sample(S, c->stream));
        if ((rc = run_lp(c, x, c->d_dvtmp, n, false, false))) return rc;
        obj.resize(n);
        if ((rc = copy_lp_outputs(c, n, obj.data(), nullptr, nullptr, nullptr, nullptr))) return rc;
        for (int i = 0; i < n; ++i) acc += invN * obj[i];
    }
    *s2 = acc;
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

// x-independent element data of the pool (rebuilt when the pool or the positions change):
// per basis p the rows of B_p^{-1}[:, row_e] over the random elements e (host CSR kptr/ke/
// kraw, e ascending) and the same as sliced ELL on the device (kslot pool-strided, absolute
// into kix/kv).  The kernels multiply the scenario deltas by coef_e(x) (d_kcoef) themselves.
int twosd::prepare_elements(twosd_ctx *c) {
    const auto t_pe0 = std::chrono::steady_clock::now();
    if (int rc0 = ensure_host_pool(c)) return rc0;
    const int m = c->L.m, k = c->k, R = c->R;
    std::vector<std::vector<int>> bycol(m);   // random elements on each row
    for (int e = 0; e < k; ++e) bycol[c->pos_row[e]].push_back(e);
    const int P = (int)c->pool.size();
    std::vector<int8_t> bt(c->L.n + m);
    HIPCHK(hipMemcpy(bt.data(), c->d_btype, bt.size(), hipMemcpyDeviceToHost));
    // pass 1: per basis and row the number of element entries; CSR / ELL / record sizes
    std::vector<int> rowcnt((size_t)P * m), width((size_t)P * R);
    std::vector<size_t> kcnt(P + 1, 0), ecnt(P + 1, 0);
    std::vector<int64_t> ccnt(P + 1, 0);
    parallel_for(P, [&](int p) {
        const PoolBasis &B = c->pool[p];
        int *rc = rowcnt.data() + (size_t)p * m;
        size_t tot = 0;
        int64_t cp = 0;   // selection records: every row active; rows of fixed (E) basics twice
        for (int i = 0; i < m; ++i) {
            int n_i = 0;
            for (int q = B.rptr[i]; q < B.rptr[i + 1]; ++q) n_i += (int)bycol[B.rcol[q]].size();
            rc[i] = n_i;
            tot += n_i;
            cp += (int64_t)(1 + n_i) * (bt[B.head[i]] == BT_E ? 2 : 1);
        }
        size_t ell = 0;
        for (int t = 0; t < R; ++t) {
            int w = 0;
            for (int l = 0; l < 64 && 64 * t + l < m; ++l) w = std::max(w, rc[64 * t + l]);
            width[(size_t)p * R + t] = w;
            ell += (size_t)w * 64;
        }
        kcnt[p + 1] = tot;
        ecnt[p + 1] = ell;
        ccnt[p + 1] = cp;
    });
    for (int p = 0; p < P; ++p) { kcnt[p + 1] += kcnt[p]; ecnt[p + 1] += ecnt[p]; ccnt[p + 1] += ccnt[p]; }
    if (kcnt[P] > INT32_MAX || ecnt[P] / 64 > INT32_MAX || ccnt[P] > INT32_MAX)
        return fail(TWOSD_E_UNSUPPORTED, "basis pool element data too large (> 2^31 entries)");
    // pass 2: rows of B_p^{-1}[:, row_e] (e ascending) as CSR (selection inputs) and sliced ELL
    // by row (x_B warm start of the LP kernel), written in place
    const size_t kz = std::max<size_t>(kcnt[P], 1), ez = std::max<size_t>(ecnt[P], 1);
    std::vector<int> kp((size_t)P * (m + 1)), ks((size_t)P * (R + 1)), cap(P + 1);
    int *ke = c->stage[STG_ELEM_KE].reserve<int>(kz), *ki = c->stage[STG_ELEM_KIX].reserve<int>(ez);
    double *kr = c->stage[STG_ELEM_KRAW].reserve<double>(kz), *kv = c->stage[STG_ELEM_KV].reserve<double>(ez);
    if (!ke || !ki || !kr || !kv) return fail(TWOSD_E_DEVICE, "pool elements: pinned staging allocation failed");
    for (int p = 0; p <= P; ++p) cap[p] = (int)ccnt[p];
    parallel_for(P, [&](int p) {
        const PoolBasis &B = c->pool[p];
        const int *rc = rowcnt.data() + (size_t)p * m;
        std::vector<std::pair<int, double>> row;
        size_t at = kcnt[p];
        const size_t e_row0 = ecnt[p] / 64;   // first ELL entry row of this basis
        size_t so = 0;                        // slot offset (entry rows) within the basis
        for (int t = 0; t <= R; ++t) {
            ks[(size_t)p * (R + 1) + t] = (int)(e_row0 + so);
            if (t < R) so += width[(size_t)p * R + t];
        }
        for (int i = 0; i < m; ++i) {
            row.clear();
            for (int q = B.rptr[i]; q < B.rptr[i + 1]; ++q)
                for (int e : bycol[B.rcol[q]]) row.push_back({e, B.rval[q]});
            std::sort(row.begin(), row.end());
            kp[(size_t)p * (m + 1) + i] = (int)at;
            for (auto &ev : row) { ke[at] = ev.first; kr[at] = ev.second; ++at; }
        }
        kp[(size_t)p * (m + 1) + m] = (int)at;
        (void)rc;
        for (int t = 0; t < R; ++t) {
            const int w = width[(size_t)p * R + t];
            const size_t r0 = (size_t)ks[(size_t)p * (R + 1) + t];
            for (int l = 0; l < 64; ++l) {
                const int i = 64 * t + l;
                const int q0 = i < m ? kp[(size_t)p * (m + 1) + i] : 0, q1 = i < m ? kp[(size_t)p * (m + 1) + i + 1] : 0;
                for (int e = 0; e < w; ++e) {
                    const bool has = q0 + e < q1;
                    ki[(r0 + e) * 64 + l] = has ? ke[q0 + e] : 0;
                    kv[(r0 + e) * 64 + l] = has ? kr[q0 + e] : 0.0;
                }
            }
        }
    });
    const auto t_pe1 = std::chrono::steady_clock::now();
    int rc;
    if (c->CH > 0 && ((rc = c->d_kslot.upload_reserve(ks)) || (rc = c->d_kix.upload_reserve(ki, ecnt[P])) ||
                      (rc = c->d_kv.upload_reserve(kv, ecnt[P]))))
        return rc;
    const auto t_pe2 = std::chrono::steady_clock::now();
    if (c->CH > 0 && P > 1) {
        // device selection-stream inputs: CSR rows of every basis, and a static record capacity
        // per basis (every row active: m row starts + all its entries)
        if ((rc = c->d_kp.upload_reserve(kp)) || (rc = c->d_ke.upload_reserve(ke, kz)) || (rc = c->d_kraw.upload_reserve(kr, kz)) ||
            (rc = c->d_sel_ptr.upload_reserve(cap)) || (rc = reserve_selection(c, P, cap[P])))
            return rc;
    }
    c->k_valid = true;
    if (getenv("TWOSD_DEBUG")) {
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "prepare_elements P=%d: build %.1f ms, upload ell %.1f ms (%zu entries), selection inputs %.1f ms\n",
                P, ms(t_pe0, t_pe1), ms(t_pe1, t_pe2), ecnt[P], ms(t_pe2, std::chrono::steady_clock::now()));
    }
    return TWOSD_OK;
}

// x_B of every pool basis at b: xbase[p][i] = sum_q B_p^{-1}[i][col_q] b[col_q] over the CSR
// rows (pool-strided brptr, MP + 1 per basis; rows >= m are empty), q ascending
__global__ void pool_xbase_kernel(int P, int MP, const int *__restrict__ brptr, const int *__restrict__ brcol,
                                  const double *__restrict__ brval, const double *__restrict__ b, double *__restrict__ xbase) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)P * MP) return;
    const size_t p = t / MP, i = t - p * MP;
    const int *rp = brptr + p * (MP + 1);
    double s = 0.0;
    int q = rp[i];
    const int q1 = rp[i + 1];
    // four entries' loads in flight together; the fmas stay in column order (same bits)
    for (; q + 4 <= q1; q += 4) {
        const int c0 = brcol[q], c1 = brcol[q + 1], c2 = brcol[q + 2], c3 = brcol[q + 3];
        const double v0 = brval[q], v1 = brval[q + 1], v2 = brval[q + 2], v3 = brval[q + 3];
        const double b0 = b[c0], b1 = b[c1], b2 = b[c2], b3 = b[c3];
        s = fma(v0, b0, s);
        s = fma(v1, b1, s);
        s = fma(v2, b2, s);
        s = fma(v3, b3, s);
    }
    for (; q < q1; ++q) s = fma(brval[q], b[brcol[q]], s);
    xbase[t] = s;
}

// primal infeasibility of a basic variable at value x (h_infeas of lp_hyper.hip, tolerance 1e-9)
__device__ __forceinline__ double dev_infeas(double x, int bt) {
    const double tol = 1e-9;
    if (bt == BT_Y || bt == BT_L) return x < -tol ? x : 0.0;
    if (bt == BT_G) return x > tol ? x : 0.0;
    return fabs(x) > tol ? x : 0.0;
}

// Selection stream of one pool basis per block (prepare_x, per x; hb0 = head * 4 + bound type): the rows of basis p that can
// turn infeasible on the training box of the deltas, ordered by their worst box infeasibility
// (largest first, row index on ties), each written as a row-start record (sign-folded
// x_B,i, the sentinel offset k * 65 * 8) followed by its element entries (e, B_p^{-1}[i][row_e]) at the basis's static capacity
// offset; rows without entries add their constant infeasibility to cinf[p] (fixed-order sum).
constexpr int kSelStreamThreads = 256;
// count weight of the selection key in units of the mean |coef_e| E|V_e - E V_e| (storm: 13.5;
// 1M bench: 0 -> 111.5 ms per step, 0.37 - 0.74 -> 105.5 - 105.8, 1.5 -> 112, 3 -> 115; ssn: no effect)
constexpr double kSelCountWeight = 0.5;
constexpr int kSelStreamRows = 1024;   // MP <= 1024 (R <= 16)
__global__ void __launch_bounds__(kSelStreamThreads) pool_selstream_kernel(
    int m, int MP, int k, const double *__restrict__ xbase, const int *__restrict__ hb0,
    const int *__restrict__ kp, const int *__restrict__ ke, const double *__restrict__ kraw, const double *__restrict__ xaux,
    int box, int order_rows, float cw, const int *__restrict__ scap, int2 *__restrict__ rec, int *__restrict__ send,
    float *__restrict__ cinf) {
    __shared__ double skey[kSelStreamRows];
    __shared__ int sidx[kSelStreamRows];
    __shared__ int soff[kSelStreamRows];
    __shared__ float cpart[kSelStreamThreads];
    __shared__ int tsum[kSelStreamThreads];
    const int p = blockIdx.x, tid = threadIdx.x;
    const double *coef = xaux + m, *lo_e = xaux + m + k, *hi_e = xaux + m + 2 * k;
    const int *kpp = kp + (size_t)p * (m + 1);
    float cf = 0.0f;
    for (int i = tid; i < kSelStreamRows; i += kSelStreamThreads) {
        double key = INFINITY;   // inactive rows sort last
        if (i < m) {
            const int t = (hb0[(size_t)p * MP + i] & 3);
            const double xv = xbase[(size_t)p * MP + i];
            const int q0 = kpp[i], q1 = kpp[i + 1];
            if (q0 == q1) {
                const double f = fabs(dev_infeas(xv, t));
                cf += (float)f + (f > 0.0 ? cw : 0.0f);
            } else {
                double worst = 0.0;
                bool active = true;
                if (box) {
                    double lo = xv, hi = xv, mag = fabs(xv);
                    for (int q = q0; q < q1; ++q) {
                        const int e = ke[q];
                        const double g = coef[e] * kraw[q];
                        const double a = g * lo_e[e], bb = g * hi_e[e];
                        lo += fmin(a, bb);
                        hi += fmax(a, bb);
                        mag += fmax(fabs(a), fabs(bb));
                    }
                    const double tol = 1e-9 + 1e-12 * mag;
                    const bool feasible_box = (t == BT_Y || t == BT_L) ? lo > tol : (t == BT_G) ? hi < -tol : false;
                    if (isfinite(lo) && isfinite(hi) && feasible_box) active = false;
                    worst = (t == BT_Y || t == BT_L) ? -lo : (t == BT_G) ? hi : fmax(fabs(lo), fabs(hi));
                    if (!isfinite(worst)) worst = HUGE_VAL;
                }
                if (active) key = order_rows ? -worst : 0.0;
            }
        }
        skey[i] = key;
        sidx[i] = i;
    }
    cpart[tid] = cf;
    __syncthreads();
    // bitonic sort of (key, row) ascending: (-worst, i) lexicographic = the host's stable sort
    for (int kk = 2; kk <= kSelStreamRows; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t2 = tid; t2 < kSelStreamRows / 2; t2 += kSelStreamThreads) {
                const int a = 2 * j * (t2 / j) + (t2 % j), b2 = a + j;
                const bool up = (a & kk) == 0;
                const double ka = skey[a], kb = skey[b2];
                const int ia = sidx[a], ib = sidx[b2];
                const bool gt = ka > kb || (ka == kb && ia > ib);
                if (gt == up) {
                    skey[a] = kb; skey[b2] = ka;
                    sidx[a] = ib; sidx[b2] = ia;
                }
            }
            __syncthreads();
        }
    }
    // records per sorted position, exclusive scan (4 consecutive positions per thread)
    constexpr int PER = kSelStreamRows / kSelStreamThreads;
    int loc[PER], run = 0;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int sp = tid * PER + u;
        const int i = sidx[sp];
        const int c = skey[sp] != INFINITY ? (1 + kpp[i + 1] - kpp[i]) * ((hb0[(size_t)p * MP + i] & 3) == BT_E ? 2 : 1) : 0;
        loc[u] = run;
        run += c;
    }
    tsum[tid] = run;
    __syncthreads();
    if (tid == 0) {   // fixed-order sums: 256 partials (records, constant-row infeasibility)
        int acc = 0;
        float cacc = 0.0f;
        for (int t = 0; t < kSelStreamThreads; ++t) {
            const int v = tsum[t];
            tsum[t] = acc;
            acc += v;
            cacc += cpart[t];
        }
        send[p] = scap[p] + acc;
        cinf[p] = cacc;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; ++u) soff[tid * PER + u] = tsum[tid] + loc[u];
    __syncthreads();
    // emit: one wave per sorted row at a time, the row's entries written by consecutive lanes
    const int lane = tid & 63, wv = tid >> 6;
    const size_t base = (size_t)scap[p];
    for (int sp = wv; sp < kSelStreamRows; sp += kSelStreamThreads / 64) {
        if (skey[sp] == INFINITY) break;   // sorted: the inactive rows are all at the end
        const int i = sidx[sp];
        const int q0 = kpp[i], q1 = kpp[i + 1];
        int2 *out = rec + base + soff[sp];
        // records are sign-folded so that the kernels' test is always "x' > tol": x' = -x for
        // Y / L basics (infeasible below 0), x for G (above 0); a fixed (E) basic is written
        // twice, with +x and -x (|x| > tol <=> one of them > tol)
        const int t = hb0[(size_t)p * MP + i] & 3;
        const int ncopy = t == BT_E ? 2 : 1;
        for (int cpy = 0; cpy < ncopy; ++cpy) {
            const float sg = (t == BT_Y || t == BT_L || cpy == 1) ? -1.0f : 1.0f;
            int2 *o = out + cpy * (1 + q1 - q0);
            // record (value bits, byte offset of the element's staged pair row e * 65 * 8; row start: the
            // offset of row k, which the selection kernels keep zeroed)
            if (lane == 0) o[0] = make_int2(__float_as_int(sg * (float)xbase[(size_t)p * MP + i]), k * 65 * 8);
            for (int q = q0 + lane; q < q1; q += 64) o[1 + q - q0] = make_int2(__float_as_int(sg * (float)kraw[q]), ke[q] * 65 * 8);
        }
    }
}

// per-x shared data: b = r - T x; per pool basis xbase_p = B_p^{-1} b (sparse rows);
// coef_e(x); with a pool, the
// selection stream (active rows that can turn infeasible on the training box of the deltas).
// Every pool basis is independent, so the per-basis work runs on host threads.
int twosd::prepare_x(twosd_ctx *c, const double *x) {
    const int m = c->L.m, MP = c->MP, k = c->k, n1 = c->n1;
    if (c->prep_valid && c->prep_x.size() == (size_t)n1 && (n1 == 0 || std::equal(c->prep_x.begin(), c->prep_x.end(), x)))
        return TWOSD_OK;
    int rc;
    const auto t_start = std::chrono::steady_clock::now();
    if (!c->k_valid && (rc = prepare_elements(c))) return rc;
    std::vector<double> b;
    rhs_at(c, x, nullptr, b);
    const int P = (int)c->pool.size();
    std::vector<double> coef(std::max(k, 1), 1.0);
    for (int e = 0; e < k; ++e) coef[e] = c->pos_col[e] < 0 ? 1.0 : -x[c->pos_col[e]];
    if ((rc = c->d_xbase.fit((size_t)P * MP))) return rc;
    if (c->CH > 0) {
        // everything per x on the device: one upload of [b, coef, box lo, box hi], x_B of every
        // pool basis, then the selection stream (pool_selstream_kernel)
        const bool sel = P > 1;
        const bool box = !c->sel_lo.empty();
        std::vector<double> aux((size_t)m + 3 * (size_t)k, 0.0);
        std::copy(b.begin(), b.end(), aux.begin());
        std::copy(coef.begin(), coef.begin() + k, aux.begin() + m);
        if (box) {
            std::copy(c->sel_lo.begin(), c->sel_lo.end(), aux.begin() + m + k);
            std::copy(c->sel_hi.begin(), c->sel_hi.end(), aux.begin() + m + 2 * k);
        }
        // re-uploaded in place: no reallocation per x
        if ((rc = c->d_xaux.fit(aux.size())) || (rc = c->d_xaux.copy_from(aux.data(), aux.size())) ||
            (rc = c->d_kcoef.fit(coef.size())) || (rc = c->d_kcoef.copy_from(coef.data(), coef.size())))
            return rc;
        const size_t tot = (size_t)P * MP;
        hipLaunchKernelGGL(pool_xbase_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, P, MP, c->d_brptr,
                           c->d_brcol, c->d_brval, c->d_xaux, c->d_xbase);
        HIPCHK(hipGetLastError());
        if (sel) {
            if (MP > kSelStreamRows) return fail(TWOSD_E_UNSUPPORTED, "pool selection: m = %d rows > %d", m, kSelStreamRows);
            // count weight of the selection key: kSelCountWeight x the mean over the random elements
            // of |coef_e(x)| E|V_e - E V_e| (one infeasible row is worth about half a typical
            // scenario perturbation), 0 without distributions.  The same on every rank.
            double sc = 0.0;
            if (c->has_dist && k > 0) {
                for (int e = 0; e < k; ++e) sc += fabs(coef[e]) * c->dist_mad[e];
                sc /= k;
            }
            c->sel_cw = (float)(kSelCountWeight * sc);
            if (const char *e = getenv("TWOSD_SEL_CW")) c->sel_cw = (float)atof(e);   // selection-key experiments
            static const bool sel_order = !getenv("TWOSD_SEL_ROWORDER") || atoi(getenv("TWOSD_SEL_ROWORDER")) != 0;   // A/B knob
            hipLaunchKernelGGL(pool_selstream_kernel, dim3(P), dim3(kSelStreamThreads), 0, c->stream, m, MP, k, c->d_xbase,
                               c->d_hb0, c->d_kp, c->d_ke, c->d_kraw, c->d_xaux, box ? 1 : 0, sel_order ? 1 : 0,
                               c->sel_cw, c->d_sel_ptr, reinterpret_cast<int2 *>(c->d_sel_code.p), c->d_sel_end, c->d_sel_cinf);
            HIPCHK(hipGetLastError());
        }
        if (getenv("TWOSD_DEBUG") && sel) {
            HIPCHK(hipStreamSynchronize(c->stream));
            std::vector<int> beg(P + 1), end(P);
            HIPCHK(hipMemcpy(beg.data(), c->d_sel_ptr, sizeof(int) * (P + 1), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(end.data(), c->d_sel_end, sizeof(int) * P, hipMemcpyDeviceToHost));
            c->sel_nnz = 0;
            for (int p = 0; p < P; ++p) c->sel_nnz += end[p] - beg[p];
            c->sel_rows = 0;
        }
    }
    c->prep_x.assign(x, x + n1);
    c->prep_valid = true;
    if (getenv("TWOSD_DEBUG")) {
        HIPCHK(hipStreamSynchronize(c->stream));
        fprintf(stderr, "prepare_x: P=%d %.3f ms (%lld selection records)\n", P,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(),
                (long long)(c->sel_nnz + c->sel_rows));
    }
    return TWOSD_OK;
}

// Warm-start selection for scenarios [0, N) at the prepared x: pick[s] = pool basis, and
// c->d_order = the scenarios grouped by pick (stable).  Flat: least key over the whole pool.
// Two-level (pool_l1 > 0): least key over pool[0, pool_l1), then over the candidates of that
// pick.  npool_override > 0: flat over pool[0, npool_override) (candidate training).
static int select_pool(twosd_ctx *c, const double *d_dv, int N, int *d_pick, int npool_override) {
    const int P = (int)c->pool.size();
    const bool two = npool_override <= 0 && c->pool_l1 > 0 && c->pool_l1 < P && c->pool_ncand > 0 && (c->d_cand || c->cand_pending);
    const int np1 = npool_override > 0 ? npool_override : two ? c->pool_l1 : P;
    int rc;
    size_t tb = 0, tb2 = 0;
    HIPCHK(sort_by_pool(d_pick, nullptr, N, P, nullptr, &tb, c->stream));
    HIPCHK(sort_by_pool(d_pick, nullptr, N, np1, nullptr, &tb2, c->stream));
    tb = std::max(tb, tb2);
    if ((size_t)N > c->d_order.cap || tb > c->d_sort_tmp.cap) {   // both at once, as one workspace
        if ((rc = c->d_order.alloc((size_t)N)) || (rc = c->d_sort_tmp.alloc(tb))) return rc;
    }
    if (two && (rc = c->d_sel_key.fit((size_t)N))) return rc;
    // partials of the chunked selections (small batches: several pool chunks per scenario tile)
    const int g1 = pool_select_split(N, np1), g2 = two ? pool_refine_split(N, c->pool_ncand) : 1;
    const size_t pneed = (size_t)std::max(g1, g2) * N;
    if (std::max(g1, g2) > 1 && ((rc = c->d_sel_pkey.fit(pneed)) || (rc = c->d_sel_ppick.fit(pneed)))) return rc;
    PoolSelParams S{};
    S.N = N; S.k = c->k; S.npool = np1; S.dv = d_dv;
    S.kcoef = c->d_kcoef;
    S.cinf = c->d_sel_cinf; S.sptr = c->d_sel_ptr; S.send = c->d_sel_end; S.rec = reinterpret_cast<const int2 *>(c->d_sel_code.p);
    S.pick = d_pick;
    S.cw = c->sel_cw;
    S.key = two ? c->d_sel_key : nullptr;
    S.pkey = g1 > 1 ? c->d_sel_pkey : nullptr;
    S.ppick = g1 > 1 ? c->d_sel_ppick : nullptr;
    HIPCHK(launch_pool_select(S, c->stream));
    if (two && c->cand_pending &&
        (rc = set_candidates(c, c->cand_pl1, c->cand_pnc, (int)c->cand_p1.size(), c->cand_p1.data(), c->cand_pf.data())))
        return rc;
    if (two) {
        HIPCHK(sort_by_pool(d_pick, c->d_order, N, np1, c->d_sort_tmp, &tb, c->stream));
        PoolRefineParams Q{};
        Q.N = N; Q.k = c->k; Q.ncand = c->pool_ncand; Q.dv = d_dv; Q.kcoef = c->d_kcoef;
        Q.cinf = c->d_sel_cinf; Q.sptr = c->d_sel_ptr; Q.send = c->d_sel_end; Q.rec = S.rec;
        Q.order = c->d_order; Q.cand = c->d_cand; Q.pick = d_pick; Q.key = c->d_sel_key; Q.cw = c->sel_cw;
        Q.pkey = g2 > 1 ? c->d_sel_pkey : nullptr;
        Q.pci = g2 > 1 ? c->d_sel_ppick : nullptr;
        HIPCHK(launch_pool_refine(Q, c->stream));
    }
    HIPCHK(sort_by_pool(d_pick, c->d_order, N, P, c->d_sort_tmp, &tb, c->stream));
    return TWOSD_OK;
}

// Launch the LP kernel over N scenarios whose deltas start at d_dv (device); results in
// c->d_obj / d_pi / d_y / d_status / d_iters [0, N).
int twosd::run_lp(twosd_ctx *c, const double *x, const double *d_dv, int N, bool want_pi, bool want_y) {
    LpRun o;
    o.want_pi = want_pi;
    o.want_y = want_y;
    return run_lp_ex(c, x, d_dv, N, o);
}

// N = scenarios of d_dv addressed by the launch (outputs obj / status / iters / pool picks are
// indexed by scenario); list mode solves only o.d_list[0, o.nlist) from their recorded picks
// and writes pi at the list position
int twosd::run_lp_ex(twosd_ctx *c, const double *x, const double *d_dv, int N, const LpRun &o) {
    const bool want_pi = o.want_pi, want_y = o.want_y;
    const bool list = o.d_list != nullptr;
    const int NL = list ? o.nlist : N;   // scenarios this launch solves
    int rc;
    if ((rc = prepare_x(c, x))) return rc;
    if (list && c->pool.size() > 1 && (size_t)N > c->d_pool_pick.cap) return fail(TWOSD_E_STATE, "LP list mode: no recorded pool picks");
    const int m = c->L.m, n = c->L.n, MP = c->MP, R = c->R;
    if (N > c->out_cap) {
        size_t cap = std::max<size_t>(N, 1024);
        if ((rc = c->d_obj.alloc(cap)) || (rc = c->d_status.alloc(cap)) || (rc = c->d_iters.alloc(cap)) ||
            (rc = c->d_ops.alloc(cap)) || (rc = c->d_etan.alloc(cap)))
            return rc;
        c->d_pi.release(); c->d_y.release();
        c->out_cap = (int)cap;
    }
    // the optional outputs, out_cap rows each, on their first use at this out_cap
    if (want_pi && (size_t)NL * m > c->d_pi.cap && (rc = c->d_pi.alloc((size_t)c->out_cap * m))) return rc;
    if (o.want_key && (size_t)N > c->d_vkey.cap && (rc = c->d_vkey.alloc((size_t)c->out_cap))) return rc;
    if (o.want_bkey && (size_t)N > c->d_bkey.cap && (rc = c->d_bkey.alloc((size_t)c->out_cap))) return rc;
    if (want_y && (size_t)N * n > c->d_y.cap && (rc = c->d_y.alloc((size_t)c->out_cap * n))) return rc;
    if (!c->d_queue && (rc = c->d_queue.alloc((size_t)kMaxQueueGroups * kQueueStride))) return rc;
    {
        // eta capacity (pivots per scenario): 2m + 32, at least 64.  256 keeps storm's two 4-wave
        // blocks per CU within the LDS; past 256 the file grows (up to 1024, in steps of 32) as far as
        // the LDS keeps the occupancy of 256 -- a scenario that needs more pivots from its pool start
        // than the file holds is retried from the primary basis (ssn 100k: 11 in 8 steps at 256)
        const int CH = c->CH;
        int kmax = c->kmax_override > 0 ? c->kmax_override : std::min(256, std::max(64, 2 * m + 32));
        if (c->kmax_override <= 0 && 2 * m + 32 > kmax) {
            const int b0 = hyper_max_blocks_per_cu(R, CH, kmax, c->k);
            for (int k2 = std::min(1024, (2 * m + 32) & ~31); k2 > kmax; k2 -= 32)
                if (hyper_max_blocks_per_cu(R, CH, k2, c->k) >= b0) { kmax = k2; break; }
        }
        // per-wave eta arena: 32 entries per row, scaled with the file past 256 pivots
        const int ecap = (int)std::min<long long>(INT32_MAX / 2, (long long)std::max(4096, 32 * MP) * std::max(256, kmax) / 256);
        int bpc = hyper_max_blocks_per_cu(R, CH, kmax, c->k);
        if (const char *e = getenv("TWOSD_BPC")) bpc = std::min(bpc, std::max(1, atoi(e)));   // diagnostics: occupancy sweep
        if (bpc < 1)
            return fail(TWOSD_E_UNSUPPORTED, "LP kernel: LDS slice too large (m2 = %d, n2 = %d; LP: %d rows, %d columns; k = %d)",
                        c->m2_user, c->n2_user, m, n, c->k);
        const int nblocks = std::max(1, std::min((NL + kWavesPerBlock - 1) / kWavesPerBlock, bpc * c->num_cus));
        const size_t slots = (size_t)nblocks * kWavesPerBlock;
        if (slots > c->earena_slots || ecap != c->earena_cap) {
            if ((rc = c->d_eidx.alloc(slots * ecap)) || (rc = c->d_evals.alloc(slots * ecap))) return rc;
            c->earena_slots = slots;
            c->earena_cap = ecap;
        }
        HIPCHK(hipMemsetAsync(c->d_queue, 0, sizeof(int) * kMaxQueueGroups * kQueueStride, c->stream));
        HyperParams H{};
        H.m = m; H.n = n; H.k = c->k; H.N = NL; H.kmax = kmax; H.ecap = ecap;
        H.kcap = o.kcap > 0 ? std::min(o.kcap, kmax) : kmax;
        H.retry = o.kcap > 0 ? 0 : 1;
        H.colptr = c->d_colptr; H.rowidx = c->d_rowidx; H.val = c->d_val; H.q = c->d_q; H.btype = c->d_btype;
        H.wcp = c->d_wcp; H.wcc = c->d_wcc; H.wcv = c->d_wcv;
        H.bcp = c->d_bcp; H.bci = c->d_bci; H.bcv = c->d_bcv;
        H.brptr = c->d_brptr; H.brcol = c->d_brcol; H.brval = c->d_brval;
        H.kslot = c->d_kslot; H.kix = c->d_kix; H.kv = c->d_kv; H.kcoef = c->d_kcoef;
        H.xbase = c->d_xbase; H.d0 = c->d_d0; H.hb0 = c->d_hb0;
        H.basic0 = c->d_basic0; H.fixedmask = c->d_fixedmask; H.ubmask = c->d_ubmask;
        H.dv = d_dv; H.eidx = c->d_eidx; H.evals = c->d_evals; H.queue = c->d_queue;
        H.qgroups = std::max(1, std::min(16, nblocks));   // two ranges per XCD (8 / 16 / 32 / 64: 143.6 / 142.7 / 142.8 / 146.3 ms, storm 1M)
        if (const char *e = getenv("TWOSD_QGROUPS")) H.qgroups = std::max(1, std::min({kMaxQueueGroups, nblocks, atoi(e)}));   // A/B knob
        H.obj = c->d_obj; H.pi = want_pi ? c->d_pi : nullptr; H.y = want_y ? c->d_y : nullptr;
        H.vkey = o.want_key ? c->d_vkey : nullptr;
        H.key_zero = 1e-12;   // = HPI_ZERO of the pi recovery (lp_hyper.hip)
        if (const char *e = getenv("TWOSD_KEY_ZERO")) H.key_zero = atof(e);   // A/B knob
        H.bkey = o.want_bkey ? c->d_bkey : nullptr;
        if (o.want_etas) {   // rows: list positions, or scenarios
            const size_t need = list ? (size_t)NL : (size_t)N;
            // eta-file offsets are 32-bit (eo_off, the device pool build): the arena of
            // 4096 entries per row must stay below 2^31 entries
            if (need * 4096 > (size_t)INT32_MAX)
                return fail(TWOSD_E_UNSUPPORTED, "eta files of %zu solves exceed the 2^31-entry arena (at most %d)", need,
                            INT32_MAX / 4096);
            // the arena: 4096 entries per row, or what an earlier training run asked for
            // (refresh_training solves again when the eta files did not fit)
            const size_t cap_need = std::max(std::max<size_t>(need, 256) * 4096, c->eo_min_cap);
            if (need > c->eo_rows || c->eo_kmax != kmax || c->eo_cap < cap_need) {
                const size_t rows = std::max<size_t>(need, 256);
                if ((rc = c->d_eo_pb.alloc(rows)) || (rc = c->d_eo_K.alloc(rows)) || (rc = c->d_eo_off.alloc(rows)) ||
                    (rc = c->d_eo_etap.alloc(rows * kmax)) || (rc = c->d_eo_etaoff.alloc(rows * (kmax + 1))) ||
                    (rc = c->d_eo_eidx.alloc(cap_need)) || (rc = c->d_eo_evals.alloc(cap_need)))
                    return rc;
                if (!c->d_eo_used && (rc = c->d_eo_used.alloc(1))) return rc;
                c->eo_rows = rows;
                c->eo_cap = cap_need;
                c->eo_kmax = kmax;
            }
            HIPCHK(hipMemsetAsync(c->d_eo_used, 0, sizeof(unsigned long long), c->stream));
            H.eo_pb = c->d_eo_pb; H.eo_K = c->d_eo_K; H.eo_off = c->d_eo_off; H.eo_etap = c->d_eo_etap;
            H.eo_etaoff = c->d_eo_etaoff; H.eo_eidx = c->d_eo_eidx; H.eo_evals = c->d_eo_evals; H.eo_used = c->d_eo_used;
            H.eo_cap = (long long)std::min<size_t>(c->eo_cap, INT32_MAX);
        }
        if (o.want_head) {   // rows: list positions, or scenarios
            const size_t need = list ? (size_t)NL : (size_t)N;
            if ((rc = c->d_head_out.fit(need * m))) return rc;
            H.head_out = c->d_head_out;
        }
        H.pi_by_pos = list ? 1 : 0;
        H.status = c->d_status; H.iters = c->d_iters; H.ops = c->d_ops; H.etan = c->d_etan;
        if (!c->d_lpstats && (rc = c->d_lpstats.alloc(6))) return rc;
        if (!list) HIPCHK(hipMemsetAsync(c->d_lpstats + 5, 0, sizeof(unsigned long long), c->stream));
        H.retries = list ? nullptr : c->d_lpstats + 5;   // a list re-solve repeats recorded picks: no retries
        if (!c->d_stamps) {
            if ((rc = c->d_stamps.alloc(16))) return rc;
            HIPCHK(hipMemset(c->d_stamps, 0, sizeof(unsigned long long) * 16));
        }
        H.stamps = c->d_stamps;
        H.npool = (int)c->pool.size();
        H.bnnz = c->d_bnnz;
        if (c->want_head && !list) {
            if ((rc = c->d_head_out.fit((size_t)N * m))) return rc;
            H.head_out = c->d_head_out;
        }
        if (H.npool > 1) {
            if (!list && (rc = c->d_pool_pick.fit((size_t)N))) return rc;
            H.pool_pick = c->d_pool_pick;
        }
        if (!list && c->d_kslot && getenv("TWOSD_DEBUG")) {
            // w, the widest ELL slot of a start basis: the x_B warm start walks w columns
            std::vector<int> ks((size_t)H.npool * (R + 1));
            HIPCHK(hipMemcpy(ks.data(), c->d_kslot, sizeof(int) * ks.size(), hipMemcpyDeviceToHost));
            std::vector<int> ws(H.npool);
            double mean = 0;
            for (int p = 0; p < H.npool; ++p) {
                int w = 0;
                for (int t = 0; t < R; ++t) w = std::max(w, ks[(size_t)p * (R + 1) + t + 1] - ks[(size_t)p * (R + 1) + t]);
                ws[p] = w;
                mean += w;
            }
            std::sort(ws.begin(), ws.end());
            fprintf(stderr, "LP start: ELL width w over %d bases: min %d, median %d, mean %.2f, p90 %d, max %d\n", H.npool, ws.front(),
                    ws[ws.size() / 2], mean / H.npool, ws[ws.size() * 9 / 10], ws.back());
        }
        HIPCHK(hipEventRecord(c->ev[0], c->stream));
        const int *order = nullptr;
        if (list) {
            order = o.d_list;
        } else if (H.npool > 1) {
            if ((rc = select_pool(c, d_dv, N, c->d_pool_pick, 0))) return rc;
            order = c->d_order;
        }
        HIPCHK(hipEventRecord(c->ev[2], c->stream));
        // one record per queue position (its scenario and start basis), so that a wave learns both
        // from its claim in one load; part of the timed LP launch.  Neither an order nor a pool:
        // position q is scenario q from the primary basis and the kernel reads no record.
        if (order || H.npool > 1) {
            if ((rc = c->d_qrec.fit(std::max<size_t>(NL, 1024)))) return rc;
            HIPCHK(launch_queue_records(order, H.npool > 1 ? c->d_pool_pick : nullptr, c->d_qrec, NL, c->stream));
            H.qrec = c->d_qrec;
        }
        HIPCHK(launch_hyper(R, CH, H, nblocks, hyper_lds_bytes(R, CH, kmax, c->k), c->stream));
        HIPCHK(hipEventRecord(c->ev[1], c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        float ms = 0, ms_sel = 0;
        hipEventElapsedTime(&ms, c->ev[2], c->ev[1]);
        hipEventElapsedTime(&ms_sel, c->ev[0], c->ev[2]);
        c->t_us[0] = 1e3 * ms;
        c->t_us[4] = 1e3 * ms_sel;
        if (list) return TWOSD_OK;
        c->last_lp_N = N;
        c->last_lp_blocks = nblocks;
        c->last_ops_width = 1;
        return TWOSD_OK;
    }
}

// batch statistics on the device (integer sums: exact, order independent): [0] pivots,
// [1] executed FMAs, [2] max pivots, [3] non-optimal scenarios
__global__ void __launch_bounds__(256) lp_stats_kernel(int N, const int *__restrict__ its, const long long *__restrict__ ops,
                                                      const int *__restrict__ st, const int *__restrict__ etan,
                                                      unsigned long long *out) {
    __shared__ unsigned long long red[4][5];
    unsigned long long a = 0, b = 0, d = 0, e = 0;
    unsigned long long mx = 0;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < N; s += gridDim.x * blockDim.x) {
        a += (unsigned long long)its[s];
        b += (unsigned long long)ops[s];
        mx = its[s] > (int)mx ? (unsigned long long)its[s] : mx;
        d += st[s] != TWOSD_LP_OPTIMAL;
        e += (unsigned long long)etan[s];
    }
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o);
        b += __shfl_down(b, o);
        d += __shfl_down(d, o);
        e += __shfl_down(e, o);
        const unsigned long long m2 = __shfl_down(mx, o);
        mx = m2 > mx ? m2 : mx;
    }
    // one set of atomics per block (per wave they serialised on five addresses: ~0.25 ms at 1M)
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[w][0] = a; red[w][1] = b; red[w][2] = mx; red[w][3] = d; red[w][4] = e;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < (int)(blockDim.x >> 6); ++v) {
            a += red[v][0]; b += red[v][1]; mx = red[v][2] > mx ? red[v][2] : mx; d += red[v][3]; e += red[v][4];
        }
        atomicAdd(&out[0], a);
        atomicAdd(&out[1], b);
        atomicMax(&out[2], mx);
        atomicAdd(&out[3], d);
        atomicAdd(&out[4], e);
    }
}

// incumbent objective of a batch: sum_s w_s obj_s and sum_s w_s (w = 1 without weights), each
// block over a fixed stride of scenarios, then a fixed tree in the block; the host adds the
// kObjBlocks partials in block order, so the sums do not depend on scheduling
constexpr int kObjBlocks = 256;
__global__ void __launch_bounds__(256) lp_obj_kernel(int N, const double *__restrict__ obj, const double *__restrict__ w,
                                                     double *__restrict__ part) {
    __shared__ double sa[256], sb[256];
    double a = 0.0, b = 0.0;
    for (int s = blockIdx.x * 256 + threadIdx.x; s < N; s += kObjBlocks * 256) {
        const double ws = w ? w[s] : 1.0;
        a = fma(ws, obj[s], a);
        b += ws;
    }
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sa[threadIdx.x] += sa[threadIdx.x + o];
            sb[threadIdx.x] += sb[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sa[0];
        part[2 * blockIdx.x + 1] = sb[0];
    }
}

// Sample moments of a batch's objectives (twosd_moments per block): block b owns the contiguous
// range [b L, min(N, (b + 1) L)), L = ceil(N / kMomBlocks), so a block's record is the moments of
// a slice of the stream and the host merges the records in block order (twosd_moments_merge).
// An entry counts when its status is optimal (PAIRED: in both arrays); the value of any other
// entry is never loaded.  Per block, over its counted entries:
//   0. the first counted index (each thread stops at its first; tree min) gives the pivot K = v[first]
//   1. n and S = sum (v - K): mean = K + S / n.  The pivot keeps the sum at the size of the
//      spread, not of the values, and makes a constant slice exact (S = 0, mean = K, m2 = 0)
//   2. sum (v - mean)^2, min, max -- the second read of the slice comes from L2
// never the one-pass sum v^2 - n mean^2, which loses 2 log10(mean / sd) digits.  PAIRED adds the
// records of b and of the per-scenario difference d = a - b (formed per entry, then reduced like
// a value): part[3 blk + 0 / 1 / 2] = a, b, d.  Every reduction is the fixed LDS tree of
// lp_obj_kernel over per-thread partials of a fixed stride: no atomics, the same bits on every run.
constexpr int kMomBlocks = 256;
template <typename T, typename Op>
__device__ __forceinline__ T mom_block_reduce(T v, T *sh, Op op) {
    __syncthreads();   // sh may still be read as the previous reduction's result
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = op(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    return sh[0];
}
template <bool PAIRED>
__global__ void __launch_bounds__(256) eval_moments_kernel(long long N, const double *__restrict__ va,
                                                           const int *__restrict__ sa, const double *__restrict__ vb,
                                                           const int *__restrict__ sb, twosd_moments *__restrict__ part) {
    constexpr int R = PAIRED ? 3 : 1;
    __shared__ double shd[256];
    __shared__ long long shi[256];
    const long long L = (N + kMomBlocks - 1) / kMomBlocks;
    const long long lo0 = (long long)blockIdx.x * L, lo = lo0 < N ? lo0 : N, hi = lo + L < N ? lo + L : N;
    const auto counted = [&](long long i) {
        return (!sa || sa[i] == TWOSD_LP_OPTIMAL) && (!PAIRED || !sb || sb[i] == TWOSD_LP_OPTIMAL);
    };
    const auto add = [](auto x, auto y) { return x + y; };
    const long long none = 0x7fffffffffffffffLL;
    long long first = none;
    for (long long i = lo + threadIdx.x; i < hi; i += 256)
        if (counted(i)) { first = i; break; }
    first = mom_block_reduce(first, shi, [](long long x, long long y) { return x < y ? x : y; });
    twosd_moments *out = part + (size_t)R * blockIdx.x;
    if (first == none) {   // an empty slice, or nothing counted: the merge's identity
        if (threadIdx.x == 0)
            for (int r = 0; r < R; ++r) out[r] = twosd_moments{0, hi - lo, 0.0, 0.0, HUGE_VAL, -HUGE_VAL};
        return;
    }
    double K[R], S[R], mean[R], q[R], mn[R], mx[R];
    K[0] = va[first];
    if (PAIRED) { K[1] = vb[first]; K[2] = K[0] - K[1]; }
    long long n = 0;
    for (int r = 0; r < R; ++r) S[r] = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        if (!counted(i)) continue;
        ++n;
        const double a = va[i];
        S[0] += a - K[0];
        if (PAIRED) {
            const double b = vb[i];
            S[1] += b - K[1];
            S[2] += (a - b) - K[2];
        }
    }
    n = mom_block_reduce(n, shi, add);
    for (int r = 0; r < R; ++r) {
        S[r] = mom_block_reduce(S[r], shd, add);
        mean[r] = K[r] + S[r] / (double)n;
        q[r] = 0.0; mn[r] = HUGE_VAL; mx[r] = -HUGE_VAL;
    }
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        if (!counted(i)) continue;
        double v[R];
        v[0] = va[i];
        if (PAIRED) { v[1] = vb[i]; v[2] = v[0] - v[1]; }
        for (int r = 0; r < R; ++r) {
            const double e = v[r] - mean[r];
            q[r] = fma(e, e, q[r]);
            mn[r] = v[r] < mn[r] ? v[r] : mn[r];
            mx[r] = v[r] > mx[r] ? v[r] : mx[r];
        }
    }
    for (int r = 0; r < R; ++r) {
        q[r] = mom_block_reduce(q[r], shd, add);
        mn[r] = mom_block_reduce(mn[r], shd, [](double x, double y) { return x < y ? x : y; });
        mx[r] = mom_block_reduce(mx[r], shd, [](double x, double y) { return x > y ? x : y; });
    }
    if (threadIdx.x == 0)
        for (int r = 0; r < R; ++r) out[r] = twosd_moments{n, (hi - lo) - n, mean[r], n > 1 ? q[r] : 0.0, mn[r], mx[r]};
}

// Group means of a variance-reduced stream (twosd_sampling): the members of a
// group of G consecutive entries are dependent, so the moments are taken over the groups' means.
// One thread per group: status[b] = optimal iff all G entries are (else the first other status),
// and only then mean[b] = K + (sum_{i < G} (v[i] - K)) / G with K = v[0], the sum in index order
// from 0.0 -- a fixed order whatever the launch shape, the pivot keeping the sum at the size of the
// spread.  The values of a group left out are never loaded (they may be NaN); its mean reads 0.
// The means are stored relative to the chunk's pivot K0 = v[0] (0 when entry 0 is not optimal or
// not finite), mean[b] = m_b - K0, and *pivot = K0: the moments kernel's block records then merge
// at the size of the spread, not of the values (the merge's d d term loses 2^-53 |mean| / sd per
// step), and the host adds K0 back to mean, min and max.  m_b - K0 is exact, and min / max the
// means' own bits, whenever m_b / 2 <= K0 <= 2 m_b.
// The paired form runs it on each array: a group counts when it is optimal in both, which the
// moments kernel sees from the two group statuses, and it forms the difference of the means itself.
__global__ void __launch_bounds__(256) group_means_kernel(long long ngroups, int G, const double *__restrict__ v,
                                                          const int *__restrict__ st, double *__restrict__ mean,
                                                          int *__restrict__ gst, double *__restrict__ pivot) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= ngroups) return;
    const double K0 = ((!st || st[0] == TWOSD_LP_OPTIMAL) && isfinite(v[0])) ? v[0] : 0.0;
    if (b == 0) *pivot = K0;
    const long long lo = b * G;
    int bad = TWOSD_LP_OPTIMAL;
    if (st)
        for (int i = 0; i < G && bad == TWOSD_LP_OPTIMAL; ++i) bad = st[lo + i];
    double m = 0.0;
    if (bad == TWOSD_LP_OPTIMAL) {
        const double K = v[lo];
        double s = 0.0;
        for (int i = 0; i < G; ++i) s = __dadd_rn(s, __dadd_rn(v[lo + i], -K));
        m = __dadd_rn(__dadd_rn(K, __ddiv_rn(s, (double)G)), -K0);
    }
    mean[b] = m;
    gst[b] = bad;
}

// Template with general bounds: the LP's outputs back into the caller's space.  yu[s][j] =
// off[j] + sign[j] * y[s][src[j]] - y[s][src2[j]] (a term with index -1 is absent: fixed columns
// have no LP column, only free ones a second), one thread per output entry, j fastest, so a wave
// writes consecutive entries of a row and reads a (nearly) consecutive run of the LP's row; and
// obj[s] += c0, the constant q.s the shift took out of the LP.  y / yu nullable (objectives only).
__global__ void __launch_bounds__(256) bounds_backmap_kernel(int N, int n2, int n_lp, const int *__restrict__ src,
                                                             const int *__restrict__ src2, const double *__restrict__ sign,
                                                             const double *__restrict__ off, const double *__restrict__ y,
                                                             double *__restrict__ yu, double c0, double *__restrict__ obj) {
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    for (size_t s = t0; s < (size_t)N; s += step) obj[s] += c0;
    if (!y) return;
    const size_t tot = (size_t)N * n2;
    for (size_t i = t0; i < tot; i += step) {
        const size_t s = i / n2;
        const int j = (int)(i - s * n2);
        const double *row = y + s * n_lp;
        const int a = src[j], b = src2[j];
        double v = off[j];
        if (a >= 0) v = fma(sign[j], row[a], v);
        if (b >= 0) v -= row[b];
        yu[i] = v;
    }
}

// d_w: the batch's scenario weights (nullable: 1.0), for the objective sum
static int copy_lp_outputs(twosd_ctx *c, int N, double *obj, double *pi, double *y, int *status, const double *d_w) {
    if (!c->d_lpstats) {
        int rc = c->d_lpstats.alloc(6);
        if (rc) return rc;
    }
    if (!c->d_objpart) {
        int rc = c->d_objpart.alloc((size_t)2 * kObjBlocks);
        if (rc) return rc;
    }
    const double *d_yout = c->d_y;
    if (c->has_bounds) {   // before the objective sum and the copies: they see the caller's values
        if (y && (size_t)N * c->n2_user > c->d_yu.cap) {
            int rc = c->d_yu.alloc((size_t)std::max(N, c->out_cap) * c->n2_user);
            if (rc) return rc;
        }
        const size_t work = y ? (size_t)N * c->n2_user : (size_t)N;
        hipLaunchKernelGGL(bounds_backmap_kernel, dim3((unsigned)std::min<size_t>(4096, (work + 255) / 256)), dim3(256), 0, c->stream, N,
                           c->n2_user, c->L.n, c->d_bm_src, c->d_bm_src2, c->d_bm_sign, c->d_bm_off, y ? c->d_y : nullptr,
                           y ? c->d_yu : nullptr, c->c0, c->d_obj);
        HIPCHK(hipGetLastError());
        d_yout = c->d_yu;
    }
    HIPCHK(hipMemsetAsync(c->d_lpstats, 0, 5 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(lp_stats_kernel, dim3((unsigned)std::min(256, (N + 255) / 256)), dim3(256), 0, c->stream, N,
                       c->d_iters, c->d_ops, c->d_status, c->d_etan, c->d_lpstats);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(lp_obj_kernel, dim3(kObjBlocks), dim3(256), 0, c->stream, N, c->d_obj, d_w, c->d_objpart);
    HIPCHK(hipGetLastError());
    unsigned long long stv[6];
    double part[2 * kObjBlocks];
    HIPCHK(hipMemcpyAsync(stv, c->d_lpstats, sizeof(stv), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(part, c->d_objpart, sizeof(part), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (obj) HIPCHK(hipMemcpy(obj, c->d_obj, sizeof(double) * N, hipMemcpyDeviceToHost));
    if (pi) HIPCHK(hipMemcpy(pi, c->d_pi, sizeof(double) * N * c->L.m, hipMemcpyDeviceToHost));
    if (y) HIPCHK(hipMemcpy(y, d_yout, sizeof(double) * N * c->n2_user, hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, c->d_status, sizeof(int) * N, hipMemcpyDeviceToHost));
    c->last_pivots_sum = (int64_t)stv[0]; c->last_ops_sum = (int64_t)stv[1]; c->last_pivots_max = (int)stv[2];
    c->last_eta_entries = (int64_t)stv[4];
    c->last_retries = (int64_t)stv[5];
    if (N >= 4096) {
        c->piv_mean_ref = (double)stv[0] / N;
        c->piv_ref_sum = (int64_t)stv[0];
        c->piv_ref_n = N;
    }
    double ow = 0.0, wt = 0.0;
    for (int b = 0; b < kObjBlocks; ++b) {
        ow += part[2 * b];
        wt += part[2 * b + 1];
    }
    c->last_obj_wsum = ow;
    c->last_obj_w = wt;
    const long long bad = (long long)stv[3];
    if (bad) return fail(TWOSD_E_LP, "%lld of %d scenario LPs not optimal (see status[])", bad, N);
    return TWOSD_OK;
}

extern "C" int twosd_last_objective(twosd_ctx *c, double *weighted_sum, double *weight_sum) {
    if (!c) return fail(TWOSD_E_ARG, "last_objective: NULL");
    if (weighted_sum) *weighted_sum = c->last_obj_wsum;
    if (weight_sum) *weight_sum = c->last_obj_w;
    return TWOSD_OK;
}

// ---- out-of-sample moments (twosd_moments_*, twosd_evaluate_moments / _paired / _ci) --------------
static const twosd_moments kMomentsEmpty = {0, 0, 0.0, 0.0, HUGE_VAL, -HUGE_VAL};

// The pairwise update of Chan, Golub and LeVeque: the one merge of the blocks' records, of the
// chunks, of the batches and of the ranks.
extern "C" int twosd_moments_merge(const twosd_moments *a, const twosd_moments *b, twosd_moments *out) {
    if (!a || !b || !out) return fail(TWOSD_E_ARG, "moments_merge: NULL");
    const twosd_moments A = *a, B = *b;   // out may alias either
    if (A.n < 0 || B.n < 0) return fail(TWOSD_E_ARG, "moments_merge: negative count");
    twosd_moments r;
    if (B.n == 0) r = A;
    else if (A.n == 0) r = B;
    else {
        const double na = (double)A.n, nb = (double)B.n, n = (double)(A.n + B.n);
        const double d = B.mean - A.mean;
        r.n = A.n + B.n;
        r.mean = A.mean + d * (nb / n);
        r.m2 = A.m2 + B.m2 + d * d * (na * nb / n);
        r.min = B.min < A.min ? B.min : A.min;
        r.max = B.max > A.max ? B.max : A.max;
    }
    r.n_bad = A.n_bad + B.n_bad;
    *out = r;
    return TWOSD_OK;
}

// moments of N device-resident values (PAIRED: also of vb and of va - vb) into out[0 .. R): the
// kernel's kMomBlocks records, one small copy, one stream sync, merged in block order
static int device_moments(twosd_ctx *c, long long N, const double *d_va, const int *d_sa, const double *d_vb,
                          const int *d_sb, twosd_moments *out) {
    const int R = d_vb ? 3 : 1;
    for (int r = 0; r < R; ++r) out[r] = kMomentsEmpty;
    if (N <= 0) return TWOSD_OK;
    if (!c->d_mompart)
        if (int rc = c->d_mompart.alloc(sizeof(twosd_moments) * 3 * kMomBlocks)) return rc;
    twosd_moments *d_part = (twosd_moments *)c->d_mompart.p;
    if (d_vb)
        hipLaunchKernelGGL(eval_moments_kernel<true>, dim3(kMomBlocks), dim3(256), 0, c->stream, N, d_va, d_sa, d_vb, d_sb, d_part);
    else
        hipLaunchKernelGGL(eval_moments_kernel<false>, dim3(kMomBlocks), dim3(256), 0, c->stream, N, d_va, d_sa, d_vb, d_sb, d_part);
    HIPCHK(hipGetLastError());
    std::vector<twosd_moments> part((size_t)R * kMomBlocks);
    HIPCHK(hipMemcpyAsync(part.data(), d_part, sizeof(twosd_moments) * part.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int b = 0; b < kMomBlocks; ++b)
        for (int r = 0; r < R; ++r) twosd_moments_merge(&out[r], &part[(size_t)R * b + r], &out[r]);
    return TWOSD_OK;
}

// device_moments over the means of groups of G consecutive entries (N a multiple of G; G = 1: the
// entries themselves): group_means_kernel into the context's group buffers, then the moments
// kernel unchanged on the N / G means and group statuses
static int device_moments_grouped(twosd_ctx *c, long long N, int G, const double *d_va, const int *d_sa, const double *d_vb,
                                  const int *d_sb, twosd_moments *out) {
    if (G <= 1 || N <= 0) return device_moments(c, N, d_va, d_sa, d_vb, d_sb, out);
    const long long ng = N / G;
    const int R = d_vb ? 2 : 1;
    int rc;
    if ((rc = c->d_gm_mean.fit((size_t)R * ng + 2)) || (rc = c->d_gm_st.fit((size_t)R * ng))) return rc;   // + the two pivots
    double *d_piv = c->d_gm_mean + (size_t)R * ng;
    const unsigned nb = (unsigned)((ng + 255) / 256);
    hipLaunchKernelGGL(group_means_kernel, dim3(nb), dim3(256), 0, c->stream, ng, G, d_va, d_sa, c->d_gm_mean.p, c->d_gm_st.p, d_piv);
    HIPCHK(hipGetLastError());
    if (d_vb) {
        hipLaunchKernelGGL(group_means_kernel, dim3(nb), dim3(256), 0, c->stream, ng, G, d_vb, d_sb, c->d_gm_mean + ng,
                           c->d_gm_st + ng, d_piv + 1);
        HIPCHK(hipGetLastError());
    }
    double piv[2] = {0.0, 0.0};
    HIPCHK(hipMemcpyAsync(piv, d_piv, sizeof(double) * (d_vb ? 2 : 1), hipMemcpyDeviceToHost, c->stream));   // device_moments drains the stream
    if ((rc = device_moments(c, ng, c->d_gm_mean, c->d_gm_st, d_vb ? c->d_gm_mean + ng : nullptr, d_vb ? c->d_gm_st + ng : nullptr, out)))
        return rc;
    const double back[3] = {piv[0], piv[1], piv[0] - piv[1]};   // the difference record is of (a - K0a) - (b - K0b)
    for (int r = 0; r < (d_vb ? 3 : 1); ++r)
        if (out[r].n > 0) { out[r].mean += back[r]; out[r].min += back[r]; out[r].max += back[r]; }
    return TWOSD_OK;
}

static int moments_of_values(twosd_ctx *c, int64_t n, int G, const double *obj, const int *status, twosd_moments *out) {
    if (!c) return fail(TWOSD_E_STATE, "moments_of_values: no context");
    if (!out || n < 0 || (n > 0 && !obj)) return fail(TWOSD_E_ARG, "moments_of_values: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if (n > 0) {
        if ((rc = c->d_ev_obj.grow((size_t)n, 0, c->stream))) return rc;
        HIPCHK(hipMemcpy(c->d_ev_obj, obj, sizeof(double) * n, hipMemcpyHostToDevice));
        if (status) {
            if ((rc = c->d_ev_st.grow((size_t)n, 0, c->stream))) return rc;
            HIPCHK(hipMemcpy(c->d_ev_st, status, sizeof(int) * n, hipMemcpyHostToDevice));
        }
    }
    return device_moments_grouped(c, n, G, c->d_ev_obj, status ? c->d_ev_st : nullptr, nullptr, nullptr, out);
}

extern "C" int twosd_moments_of_values(twosd_ctx *c, int64_t n, const double *obj, const int *status, twosd_moments *out) {
    return moments_of_values(c, n, 1, obj, status, out);
}

extern "C" int twosd_moments_of_values_grouped(twosd_ctx *c, int64_t n, int G, const double *obj, const int *status,
                                               twosd_moments *out) {
    if (G < 1 || G > 256) return fail(TWOSD_E_ARG, "moments_of_values_grouped: need 1 <= G <= 256, not %d", G);
    if (n > 0 && n % G) return fail(TWOSD_E_ARG, "moments_of_values_grouped: n = %lld is no multiple of G = %d", (long long)n, G);
    return moments_of_values(c, n, G, obj, status, out);
}

// scenarios per evaluate chunk; for a plan with G > 1 rounded down to whole groups (at least one)
static int64_t eval_chunk_size(int G) {
    int64_t chunk = 1 << 20;
    if (const char *e = getenv("TWOSD_EVAL_CHUNK")) chunk = std::min<int64_t>(std::max<int64_t>(atoll(e), 1), 1 << 24);   // test hook
    if (G > 1) chunk = std::max<int64_t>(chunk / G * G, G);
    return chunk;
}

// the sampling plan of an evaluate call: (mode, group) of twosd_sampling, i.i.d. by default
struct EvalPlan { int mode = TWOSD_SAMPLING_IID, G = 1; };

// scenarios [at, at + n) of stream `seed` drawn into d_dvtmp and solved at x; copy_lp_outputs adds
// the bounds' constant to d_obj and keeps the last-LP statistics current (nothing is copied out).
// TWOSD_OK, or TWOSD_E_LP with d_obj / d_status still set, or a failure.
static int eval_solve_chunk(twosd_ctx *c, const double *x, int64_t at, int n, uint64_t seed, const EvalPlan &pl) {
    const int k = c->k;
    int rc;
    if ((rc = c->d_dvtmp.grow((size_t)n * std::max(k, 1), 0, c->stream))) return rc;
    SampleParams S{};
    S.N = n; S.k = k; S.seed = seed; S.first_index = (unsigned long long)at;
    S.kind = c->d_dist_kind; S.off = c->d_dist_off; S.val = c->d_dist_val; S.prob = c->d_dist_prob;
    S.p0 = c->d_dist_p0; S.p1 = c->d_dist_p1; S.tmpl = c->d_dist_tmpl; S.out = c->d_dvtmp;
    HIPCHK(launch_sample_plan(S, pl.mode, pl.G, c->stream));
    if ((rc = run_lp(c, x, c->d_dvtmp, n, false, false))) return rc;
    return copy_lp_outputs(c, n, nullptr, nullptr, nullptr, nullptr, nullptr);
}

static int eval_check_state(twosd_ctx *c, const char *who) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "%s: no template", who);
    if (!c->has_basis) return fail(TWOSD_E_STATE, "%s: no warm-start basis", who);
    if (!c->has_dist) return fail(TWOSD_E_STATE, "%s: no distributions (twosd_set_distributions)", who);
    return TWOSD_OK;
}

// moments over [first, first + count) at xa (xb: the paired form, out[0 .. 3) = a, b, a - b);
// *lp_bad: some LP was not optimal (counted in n_bad; not a failure here).  Under a plan with
// G > 1 (first and count whole groups) the moments are of the group means, n / n_bad in groups.
static int eval_moments_range(twosd_ctx *c, const double *xa, const double *xb, int64_t first, int64_t count, uint64_t seed,
                              twosd_moments *out, bool *lp_bad, const EvalPlan &pl = EvalPlan()) {
    const int R = xb ? 3 : 1;
    const int64_t chunk = eval_chunk_size(pl.G);
    for (int r = 0; r < R; ++r) out[r] = kMomentsEmpty;
    for (int64_t at = 0; at < count; at += chunk) {
        const int n = (int)std::min(chunk, count - at);
        int rc = eval_solve_chunk(c, xa, first + at, n, seed, pl);
        if (rc == TWOSD_E_LP) *lp_bad = true;
        else if (rc) return rc;
        twosd_moments m[3];
        if (xb) {
            if ((rc = c->d_ev_obj.grow((size_t)n, 0, c->stream)) ||
                (rc = c->d_ev_st.grow((size_t)n, 0, c->stream)))
                return rc;
            HIPCHK(hipMemcpyAsync(c->d_ev_obj, c->d_obj, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(c->d_ev_st, c->d_status, sizeof(int) * n, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));   // the next solve may reallocate d_obj / d_status
            rc = eval_solve_chunk(c, xb, first + at, n, seed, pl);
            if (rc == TWOSD_E_LP) *lp_bad = true;
            else if (rc) return rc;
            if ((rc = device_moments_grouped(c, n, pl.G, c->d_ev_obj, c->d_ev_st, c->d_obj, c->d_status, m))) return rc;
        } else if ((rc = device_moments_grouped(c, n, pl.G, c->d_obj, c->d_status, nullptr, nullptr, m)))
            return rc;
        for (int r = 0; r < R; ++r) twosd_moments_merge(&out[r], &m[r], &out[r]);
    }
    return TWOSD_OK;
}

static int eval_lp_result(bool lp_bad, const twosd_moments &m, const char *who, int G = 1) {
    if (!lp_bad) return TWOSD_OK;
    if (G > 1)
        return fail(TWOSD_E_LP, "%s: %lld of %lld scenario groups hold an LP that is not optimal (left out of the moments, see n_bad)",
                    who, (long long)m.n_bad, (long long)(m.n + m.n_bad));
    return fail(TWOSD_E_LP, "%s: %lld of %lld scenario LPs not optimal (left out of the moments, see n_bad)", who,
                (long long)m.n_bad, (long long)(m.n + m.n_bad));
}

// the plan of an evaluate call, with `first` and `count` checked for whole groups
static int eval_plan(const twosd_sampling *plan, const char *who, int64_t first, int64_t count, const char *count_name,
                     EvalPlan *pl) {
    int rc;
    if ((rc = sampling_plan(plan, who, &pl->mode, &pl->G))) return rc;
    if (first >= 0 && (rc = whole_groups(who, "first", (unsigned long long)first, pl->G))) return rc;
    if (count >= 0 && (rc = whole_groups(who, count_name, (unsigned long long)count, pl->G))) return rc;
    return TWOSD_OK;
}

static int evaluate_moments(twosd_ctx *c, const double *x, int64_t first, int64_t count, uint64_t seed, twosd_moments *out,
                            const EvalPlan &pl) {
    int rc = eval_check_state(c, "evaluate_moments");
    if (rc) return rc;
    if (!out || first < 0 || count < 0 || (c->n1 > 0 && !x)) return fail(TWOSD_E_ARG, "evaluate_moments: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    bool lp_bad = false;
    if ((rc = eval_moments_range(c, x, nullptr, first, count, seed, out, &lp_bad, pl))) return rc;
    return eval_lp_result(lp_bad, *out, "evaluate_moments", pl.G);
}

extern "C" int twosd_evaluate_moments(twosd_ctx *c, const double *x, int64_t first, int64_t count, uint64_t seed,
                                      twosd_moments *out) {
    return evaluate_moments(c, x, first, count, seed, out, EvalPlan());
}

extern "C" int twosd_evaluate_moments_vr(twosd_ctx *c, const double *x, int64_t first, int64_t count, uint64_t seed,
                                         twosd_moments *out, const twosd_sampling *plan) {
    EvalPlan pl;
    if (int rc = eval_plan(plan, "evaluate_moments", first, count, "count", &pl)) return rc;
    return evaluate_moments(c, x, first, count, seed, out, pl);
}

static int evaluate_paired(twosd_ctx *c, const double *xa, const double *xb, int64_t first, int64_t count, uint64_t seed,
                           twosd_moments *a, twosd_moments *b, twosd_moments *diff, const EvalPlan &pl) {
    int rc = eval_check_state(c, "evaluate_paired");
    if (rc) return rc;
    if (!a || !b || !diff || first < 0 || count < 0 || !xa || !xb) return fail(TWOSD_E_ARG, "evaluate_paired: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    bool lp_bad = false;
    twosd_moments m[3];
    if ((rc = eval_moments_range(c, xa, xb, first, count, seed, m, &lp_bad, pl))) return rc;
    *a = m[0]; *b = m[1]; *diff = m[2];
    return eval_lp_result(lp_bad, m[0], "evaluate_paired", pl.G);
}

extern "C" int twosd_evaluate_paired(twosd_ctx *c, const double *xa, const double *xb, int64_t first, int64_t count,
                                     uint64_t seed, twosd_moments *a, twosd_moments *b, twosd_moments *diff) {
    return evaluate_paired(c, xa, xb, first, count, seed, a, b, diff, EvalPlan());
}

extern "C" int twosd_evaluate_paired_vr(twosd_ctx *c, const double *xa, const double *xb, int64_t first, int64_t count,
                                        uint64_t seed, twosd_moments *a, twosd_moments *b, twosd_moments *diff,
                                        const twosd_sampling *plan) {
    EvalPlan pl;
    if (int rc = eval_plan(plan, "evaluate_paired", first, count, "count", &pl)) return rc;
    return evaluate_paired(c, xa, xb, first, count, seed, a, b, diff, pl);
}

static int evaluate_ci(twosd_ctx *c, const double *x, uint64_t seed, int64_t first, int64_t batch, int64_t n_max, double z,
                       double rel_tol, double abs_tol, double offset, twosd_moments *out, double *half_width, int *converged,
                       const EvalPlan &pl) {
    if (!out || !half_width || !converged || first < 0) return fail(TWOSD_E_ARG, "evaluate_ci: bad arguments");
    if (batch < 2 || n_max < batch) return fail(TWOSD_E_ARG, "evaluate_ci: need 2 <= batch <= n_max (batch %lld, n_max %lld)", (long long)batch, (long long)n_max);
    if (!(z > 0.0) || !(rel_tol >= 0.0) || !(abs_tol >= 0.0) || !std::isfinite(offset))
        return fail(TWOSD_E_ARG, "evaluate_ci: need z > 0, tolerances >= 0 and a finite offset");
    int rc = eval_check_state(c, "evaluate_ci");
    if (rc) return rc;
    if (c->n1 > 0 && !x) return fail(TWOSD_E_ARG, "evaluate_ci: x required");
    HIPCHK(hipSetDevice(c->device));
    twosd_moments acc = kMomentsEmpty;
    bool lp_bad = false;
    double hw = HUGE_VAL;
    int conv = 0;
    for (int64_t done = 0; done < n_max && !conv; ) {
        const int64_t cnt = std::min(batch, n_max - done);
        twosd_moments m;
        if ((rc = eval_moments_range(c, x, nullptr, first + done, cnt, seed, &m, &lp_bad, pl))) return rc;
        twosd_moments_merge(&acc, &m, &acc);
        done += cnt;
        if (acc.n >= 2) {
            hw = z * std::sqrt(acc.m2 / (double)(acc.n - 1) / (double)acc.n);
            conv = hw <= std::max(abs_tol, rel_tol * std::fabs(offset + acc.mean));
        }
    }
    *out = acc;
    *half_width = hw;
    *converged = conv;
    return eval_lp_result(lp_bad, acc, "evaluate_ci", pl.G);
}

extern "C" int twosd_evaluate_ci(twosd_ctx *c, const double *x, uint64_t seed, int64_t first, int64_t batch, int64_t n_max,
                                 double z, double rel_tol, double abs_tol, double offset, twosd_moments *out,
                                 double *half_width, int *converged) {
    return evaluate_ci(c, x, seed, first, batch, n_max, z, rel_tol, abs_tol, offset, out, half_width, converged, EvalPlan());
}

// the rule of twosd_evaluate_ci on the group moments: its scenario counts (done, n_max, batch) stay
// in scenarios, acc.n / acc.n_bad are groups
extern "C" int twosd_evaluate_ci_vr(twosd_ctx *c, const double *x, uint64_t seed, int64_t first, int64_t batch, int64_t n_max,
                                    double z, double rel_tol, double abs_tol, double offset, twosd_moments *out,
                                    double *half_width, int *converged, const twosd_sampling *plan) {
    EvalPlan pl;
    if (int rc = eval_plan(plan, "evaluate_ci", first, batch, "batch", &pl)) return rc;
    if (pl.G > 1) {
        if (batch / pl.G < 2)
            return fail(TWOSD_E_ARG, "evaluate_ci: batch = %lld holds fewer than 2 groups of %d", (long long)batch, pl.G);
        n_max = n_max / pl.G * pl.G;
    }
    return evaluate_ci(c, x, seed, first, batch, n_max, z, rel_tol, abs_tol, offset, out, half_width, converged, pl);
}

extern "C" int twosd_solve_batch(twosd_ctx *c, int epi, const double *x, int first, int count, double *obj,
                                 double *pi, double *y, int *status) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "solve_batch: no template");
    if (!c->has_basis) return fail(TWOSD_E_STATE, "solve_batch: no warm-start basis (twosd_compute_basis / twosd_set_basis)");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "solve_batch: epigraph %d does not exist", epi);
    const EpiDevice &E = c->epis[epi];
    if (first < 0 || count < 0 || first + count > E.count) return fail(TWOSD_E_ARG, "solve_batch: range [%d,%d) outside %d scenarios", first, first + count, E.count);
    if (!obj || !status || (c->n1 > 0 && !x)) return fail(TWOSD_E_ARG, "solve_batch: obj/status/x required");
    if (count == 0) return TWOSD_OK;
    HIPCHK(hipSetDevice(c->device));
    int rc = run_lp(c, x, E.d_dv + (size_t)first * c->k, count, pi != nullptr, y != nullptr);
    if (rc) return rc;
    return copy_lp_outputs(c, count, obj, pi, y, status, E.d_w + first);
}

extern "C" int twosd_solve_values(twosd_ctx *c, const double *x, int N, const double *values, double *obj, double *pi,
                                  double *y, int *status) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "solve_values: no template");
    if (!c->has_basis) return fail(TWOSD_E_STATE, "solve_values: no warm-start basis");
    if (N < 0 || (N > 0 && c->k > 0 && !values) || !obj || !status || (c->n1 > 0 && !x)) return fail(TWOSD_E_ARG, "solve_values: bad arguments");
    if (N == 0) return TWOSD_OK;
    HIPCHK(hipSetDevice(c->device));
    const int k = c->k;
    std::vector<double> dv((size_t)N * std::max(k, 1), 0.0);
    for (int s = 0; s < N; ++s)
        for (int e = 0; e < k; ++e) dv[(size_t)s * k + e] = values[(size_t)s * k + e] - template_value(c, e);
    int rc;
    if ((rc = c->d_dvtmp.grow((size_t)N * std::max(k, 1), 0, c->stream))) return rc;
    HIPCHK(hipMemcpy(c->d_dvtmp, dv.data(), sizeof(double) * dv.size(), hipMemcpyHostToDevice));
    if ((rc = run_lp(c, x, c->d_dvtmp, N, pi != nullptr, y != nullptr))) return rc;
    return copy_lp_outputs(c, N, obj, pi, y, status, nullptr);
}

extern "C" int twosd_last_timings(twosd_ctx *c, double *us5) {
    if (!c || !us5) return fail(TWOSD_E_ARG, "last_timings: NULL");
    for (int i = 0; i < 5; ++i) us5[i] = c->t_us[i];
    return TWOSD_OK;
}

extern "C" int twosd_last_lp_eta_entries(twosd_ctx *c, int64_t *entries, int64_t *retries) {
    if (!c || !entries) return fail(TWOSD_E_ARG, "last_lp_eta_entries: NULL");
    *entries = c->last_eta_entries;
    if (retries) *retries = c->last_retries;
    return TWOSD_OK;
}

extern "C" int twosd_last_lp_stats(twosd_ctx *c, int64_t *sum, int *mx) {
    if (!c) return fail(TWOSD_E_ARG, "last_lp_stats: NULL");
    if (sum) *sum = c->last_pivots_sum;
    if (mx) *mx = c->last_pivots_max;
    return TWOSD_OK;
}

extern "C" int twosd_last_lp_iters(twosd_ctx *c, int N, int *iters, int *status) {
    if (!c || N < 0 || N > c->out_cap || !c->d_iters) return fail(TWOSD_E_ARG, "last_lp_iters: N = %d outside the last batch", N);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (iters) HIPCHK(hipMemcpy(iters, c->d_iters, sizeof(int) * N, hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, c->d_status, sizeof(int) * N, hipMemcpyDeviceToHost));
    return TWOSD_OK;
}

extern "C" int twosd_debug_stamps(twosd_ctx *c, uint64_t *out10, int reset) {
    if (!c || !out10) return fail(TWOSD_E_ARG, "debug_stamps: NULL");
    for (int i = 0; i < 10; ++i) out10[i] = 0;
    if (!c->d_stamps) return TWOSD_OK;
    HIPCHK(hipMemcpy(out10, c->d_stamps, sizeof(uint64_t) * 10, hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(c->d_stamps, 0, sizeof(uint64_t) * 16));
    return TWOSD_OK;
}

extern "C" int twosd_last_lp_ops(twosd_ctx *c, int64_t *row_ops, int *row_width) {
    if (!c) return fail(TWOSD_E_ARG, "last_lp_ops: NULL");
    if (row_ops) *row_ops = c->last_ops_sum;
    if (row_width) *row_width = c->last_ops_width;
    return TWOSD_OK;
}

// rows list[0..U) of pi (m doubles each) gathered in list order (the push of a full-mode solve_push)
__global__ void gather_rows_kernel(int U, int m, const int *__restrict__ list, const double *__restrict__ pi, double *__restrict__ out) {
    const size_t tot = (size_t)U * m;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) {
        const int u = (int)(i / m), r = (int)(i % m);
        out[i] = pi[(size_t)list[u] * m + r];
    }
}

// non-optimal statuses among the scenarios of a list-mode re-solve (status is by scenario)
__global__ void list_status_kernel(int U, const int *__restrict__ list, const int *__restrict__ st,
                                   unsigned long long *bad) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < U; i += gridDim.x * blockDim.x)
        if (st[list[i]] != TWOSD_LP_OPTIMAL) atomicAdd(bad, 1ull);
}

extern "C" int twosd_solve_push(twosd_ctx *c, int epi, const double *x, int first, int count, double *obj, int *status,
                                int *new_size) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "solve_push: no template");
    if (!c->has_basis) return fail(TWOSD_E_STATE, "solve_push: no warm-start basis");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "solve_push: epigraph %d does not exist", epi);
    const EpiDevice &E = c->epis[epi];
    if (first < 0 || count < 0 || first + count > E.count) return fail(TWOSD_E_ARG, "solve_push: range outside the epigraph");
    if (c->n1 > 0 && !x) return fail(TWOSD_E_ARG, "solve_push: x is NULL");
    if (count == 0) { if (new_size) *new_size = c->dvs.size; return TWOSD_OK; }
    HIPCHK(hipSetDevice(c->device));
    const double *d_dv = E.d_dv + (size_t)first * c->k;
    // TWOSD_PUSH_ALL=1: recover and push the dual of every scenario (the pre-key path, kept for
    // the equivalence test); default: vertex keys, first occurrences, re-solve of those only
    const bool all = getenv("TWOSD_PUSH_ALL") && atoi(getenv("TWOSD_PUSH_ALL")) != 0;
    // Full mode: the main pass recovers every scenario's dual (and its key), and the representatives'
    // rows are gathered from it -- the same rows the re-solve would produce (same start, same pivots,
    // same recovery), without solving them twice.  Chosen when the last keyed push re-solved more
    // than a quarter of its scenarios (ssn: ~every scenario its own vertex; storm: < 1 %).
    // TWOSD_PUSH_MODE: 0 auto (default), 1 always re-solve, 2 always full.
    const int pmode = getenv("TWOSD_PUSH_MODE") ? atoi(getenv("TWOSD_PUSH_MODE")) : 0;
    const bool full = !all && (pmode == 2 || (pmode == 0 && c->push_rep_frac > 0.25));
    c->last_push_full = full ? 1 : 0;
    LpRun o;
    o.want_pi = all || full;
    o.want_key = !all;
    int rc = run_lp_ex(c, x, d_dv, count, o);
    if (rc) return rc;
    const double t_lp = c->t_us[0], t_sel = c->t_us[4];
    rc = copy_lp_outputs(c, count, obj, nullptr, nullptr, status, E.d_w + first);
    if (rc) return rc;   // some LP not optimal: nothing pushed
    const double obj_wsum = c->last_obj_wsum, obj_w = c->last_obj_w;
    const int64_t piv_sum = c->last_pivots_sum, ops_sum = c->last_ops_sum, eta_sum = c->last_eta_entries;
    const int64_t retries = c->last_retries;
    const int piv_max = c->last_pivots_max;
    float ms = 0, ms_key = 0;
    if (all) {
        HIPCHK(hipEventRecord(c->ev[2], c->stream));
        if ((rc = dvs_push_device(c, count, c->d_pi, nullptr))) return rc;
        HIPCHK(hipEventRecord(c->ev[3], c->stream));
        HIPCHK(hipEventSynchronize(c->ev[3]));
        hipEventElapsedTime(&ms, c->ev[2], c->ev[3]);
        c->last_push_reps = count;
    } else {
        HIPCHK(hipEventRecord(c->ev[5], c->stream));
        const int *d_list = nullptr;
        int U = 0;
        if ((rc = vkey_first_occurrences(c, count, c->d_vkey, c->d_status, &d_list, &U))) return rc;
        HIPCHK(hipEventRecord(c->ev[6], c->stream));
        HIPCHK(hipEventSynchronize(c->ev[6]));
        hipEventElapsedTime(&ms_key, c->ev[5], c->ev[6]);
        c->last_push_reps = U;
        c->push_rep_frac = (double)U / count;
        if (U > 0 && full) {
            const int m = c->L.m;
            if ((rc = c->d_pi_rep.fit((size_t)U * m))) return rc;
            hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)std::min<size_t>(4096, ((size_t)U * m + 255) / 256)), dim3(256), 0,
                               c->stream, U, m, d_list, c->d_pi, c->d_pi_rep);
            HIPCHK(hipGetLastError());
            c->t_us[0] = t_lp;
            HIPCHK(hipEventRecord(c->ev[2], c->stream));
            if ((rc = dvs_push_device(c, U, c->d_pi_rep, nullptr))) return rc;
            HIPCHK(hipEventRecord(c->ev[3], c->stream));
            HIPCHK(hipEventSynchronize(c->ev[3]));
            hipEventElapsedTime(&ms, c->ev[2], c->ev[3]);
        } else if (U > 0) {
            LpRun r;
            r.want_pi = true;
            r.d_list = d_list;
            r.nlist = U;
            if ((rc = run_lp_ex(c, x, d_dv, count, r))) return rc;
            // the re-solve starts every representative from its recorded pick and repeats its
            // optimal solve; should one ever end otherwise, its pi row must not reach V
            HIPCHK(hipMemsetAsync(c->d_lpstats, 0, sizeof(unsigned long long), c->stream));
            hipLaunchKernelGGL(list_status_kernel, dim3((unsigned)std::min(256, (U + 255) / 256)), dim3(256), 0, c->stream, U,
                               d_list, c->d_status, c->d_lpstats);
            HIPCHK(hipGetLastError());
            unsigned long long bad = 0;
            HIPCHK(hipMemcpyAsync(&bad, c->d_lpstats, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            if (bad) return fail(TWOSD_E_LP, "solve_push: %llu of %d re-solved representatives not optimal; nothing pushed", bad, U);
            c->t_us[0] += t_lp;   // LP kernel time of the batch: main pass + representatives
            HIPCHK(hipEventRecord(c->ev[2], c->stream));
            if ((rc = dvs_push_device(c, U, c->d_pi, nullptr))) return rc;
            HIPCHK(hipEventRecord(c->ev[3], c->stream));
            HIPCHK(hipEventSynchronize(c->ev[3]));
            hipEventElapsedTime(&ms, c->ev[2], c->ev[3]);
        } else {
            c->t_us[0] = t_lp;
        }
        c->t_us[4] = t_sel;
        c->last_pivots_sum = piv_sum; c->last_ops_sum = ops_sum; c->last_pivots_max = piv_max;
        c->last_eta_entries = eta_sum;
        c->last_retries = retries;
    }
    c->last_obj_wsum = obj_wsum; c->last_obj_w = obj_w;   // of the batch, not of the representatives' re-solve
    c->t_us[1] = 1e3 * (ms + ms_key);
    if (new_size) *new_size = c->dvs.size;
    return TWOSD_OK;
}

extern "C" int twosd_last_push_mode(twosd_ctx *c, int *full) {
    if (!c || !full) return fail(TWOSD_E_ARG, "last_push_mode: NULL");
    *full = c->last_push_full;
    return TWOSD_OK;
}

extern "C" int twosd_last_push_reps(twosd_ctx *c, int *reps) {
    if (!c || !reps) return fail(TWOSD_E_ARG, "last_push_reps: NULL");
    *reps = c->last_push_reps;
    return TWOSD_OK;
}
