// lintr_tables.h -- correlated continuous elements ("LINTR blocks", SMPS BLOCKS LINTR, DESIGN.md
// §5.11) of the scenario sampler: the tables a set of LINTR blocks becomes and their validation.
// No HIP in here: api.hip builds the tables, lintr.hip uploads them, and
// tests/native/lintr_tables_check.cpp includes this file alone and checks it on the CPU.
//
// A block is an ordered member list e_0 .. e_{n-1} (indices into the random-element layout, in the
// caller's order), one constant c_j per member, q >= 1 latent variables (DISCRETE, NORMAL or
// UNIFORM, as twosd_set_distributions reads an element) and a sparse n x q matrix H in CSR.  The
// latents of all blocks are numbered 0 .. Q-1 in block order; latent l draws as element k + l of
// an independent layout of k + Q elements.  Member j is
//     v = c_j; for each entry (l, h) of row j in order: v = v + (h * xi_l)     (no fma)
// The tables keep the entries as given (explicit zeros included), with the block-local columns
// turned into global latent numbers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

namespace twosd {
#pragma GCC visibility push(hidden)

constexpr int kDistLintr = 4;   // kind of a LINTR member (TWOSD_DIST_LINTR)

// the caller's arrays (twosd_lintr of twosd_hip.h, field for field)
struct LintrSpec {
    int nblocks;
    const int *member_off, *members;      // nblocks + 1; M = member_off[nblocks]
    const double *constants;              // M
    const int *latent_off;                // nblocks + 1; Q = latent_off[nblocks]
    const int *latent_kind, *latent_nsupport;           // Q
    const double *latent_values, *latent_probs;         // sum of nsupport over the DISCRETE latents
    const double *latent_param0, *latent_param1;        // Q
    const int *row_ptr;                   // M + 1, one CSR over the member rows of all blocks
    const int *col;                       // row_ptr[M]: latent of the row's block, in [0, q)
    const double *val;                    // row_ptr[M]
};

// what lintr_tables_build returns; *where is the block (LT_E_OFFSETS .. LT_E_COEF), the element
// (LT_E_NO_BLOCK) or the global latent (LT_E_LATENT_*) it is about
enum LintrErr : int {
    LT_OK = 0,
    LT_E_NULL,            // a needed array is NULL, k < 0 or nblocks < 0
    LT_E_OFFSETS,         // member_off[0], latent_off[0] or row_ptr[0] is not 0, or row_ptr decreases
    LT_E_EMPTY_BLOCK,     // a block without members
    LT_E_NLATENT,         // a block with q < 1
    LT_E_TOO_LARGE,       // k + Q >= 2^31, or the latents' supports past 2^31 - 1 entries
    LT_E_MEMBER_RANGE,    // a member index outside [0, k)
    LT_E_MEMBER_KIND,     // a member whose kind is not kDistLintr
    LT_E_MEMBER_TWICE,    // an element in two blocks, or twice in one
    LT_E_NO_BLOCK,        // an element of kind kDistLintr that is in no block
    LT_E_COLUMN,          // a CSR column outside [0, q), or columns not strictly ascending in a row
    LT_E_CONSTANT,        // a non-finite constant
    LT_E_COEF,            // a non-finite coefficient
    LT_E_LATENT_KIND,     // a latent whose kind is not 0, 1 or 2
    LT_E_LATENT_SUPPORT,  // a DISCRETE latent with an empty support, repeated values or a negative probability
    LT_E_LATENT_VARIANCE  // a NORMAL latent with a negative variance
};

inline const char *lintr_err_text(int err) {
    switch (err) {
    case LT_OK: return "ok";
    case LT_E_NULL: return "NULL argument or negative count";
    case LT_E_OFFSETS: return "offsets do not start at 0 or row_ptr decreases";
    case LT_E_EMPTY_BLOCK: return "block without members";
    case LT_E_NLATENT: return "block with fewer than one latent variable";
    case LT_E_TOO_LARGE: return "k + Q or the latents' supports past 2^31 - 1";
    case LT_E_MEMBER_RANGE: return "member index outside [0, k)";
    case LT_E_MEMBER_KIND: return "member whose kind is not 4 (LINTR member)";
    case LT_E_MEMBER_TWICE: return "element in two blocks or twice in one";
    case LT_E_NO_BLOCK: return "element of kind 4 (LINTR member) in no LINTR block";
    case LT_E_COLUMN: return "CSR column outside [0, q) or not strictly ascending within its row";
    case LT_E_CONSTANT: return "non-finite constant";
    case LT_E_COEF: return "non-finite coefficient";
    case LT_E_LATENT_KIND: return "latent of unknown kind";
    case LT_E_LATENT_SUPPORT: return "DISCRETE latent with an empty support, repeated values or a negative probability";
    case LT_E_LATENT_VARIANCE: return "NORMAL latent with a negative variance";
    }
    return "unknown error";
}

struct LintrTables {
    int M = 0, Q = 0;                    // member rows and latents of all blocks
    std::vector<int> blk, row;           // k: block (-1 outside one) and row (its index among the M rows) of element e
    std::vector<int> elem;               // M: the row's element
    std::vector<double> c;               // M: the row's constant
    std::vector<int> rptr, col;          // M + 1, nnz: CSR, columns are global latent numbers
    std::vector<double> h;               // nnz
    // the latents as an independent layout of Q elements (SampleParams of the latent pass)
    std::vector<int> lkind, loff, lword; // Q, Q + 1, Q: kind, DISCRETE support range, element word k + l
    std::vector<double> lval, lprob;     // DISCRETE supports, ascending by value, and probabilities
    std::vector<double> lp0, lp1;        // Q: NORMAL mean / sd, UNIFORM left / right
    std::vector<double> lvar;            // Q: Var xi_l (DISCRETE: under p / sum p)
};

// Checks the caller's LINTR blocks against kind[k] and builds the tables.  The shapes (offsets,
// k + Q) are checked before any array of M, Q or nnz entries is read, and those are read only
// inside the lengths the shapes give.  T is written on LT_OK only.
inline int lintr_tables_build(int k, const int *kind, const LintrSpec &L, LintrTables &T, int *where) {
    const auto bad = [&](int code, int w) { if (where) *where = w; return code; };
    const int nb = L.nblocks;
    if (k < 0 || nb < 0 || (k > 0 && !kind)) return bad(LT_E_NULL, -1);
    if (nb > 0 && (!L.member_off || !L.members || !L.constants || !L.latent_off || !L.latent_kind || !L.latent_nsupport ||
                   !L.latent_param0 || !L.latent_param1 || !L.row_ptr))
        return bad(LT_E_NULL, -1);
    LintrTables N;
    N.blk.assign(k, -1); N.row.assign(k, -1);
    if (nb > 0 && (L.member_off[0] != 0 || L.latent_off[0] != 0)) return bad(LT_E_OFFSETS, 0);
    for (int b = 0; b < nb; ++b) {
        if ((long long)L.member_off[b + 1] - L.member_off[b] < 1) return bad(LT_E_EMPTY_BLOCK, b);
        if ((long long)L.latent_off[b + 1] - L.latent_off[b] < 1) return bad(LT_E_NLATENT, b);
    }
    N.M = nb ? L.member_off[nb] : 0;
    N.Q = nb ? L.latent_off[nb] : 0;
    if ((long long)k + N.Q > (long long)INT32_MAX) return bad(LT_E_TOO_LARGE, nb - 1);   // latent words k + l stay below 2^31
    const int M = N.M, Q = N.Q;
    // members
    N.elem.resize(M); N.c.resize(M);
    for (int b = 0; b < nb; ++b)
        for (int m = L.member_off[b]; m < L.member_off[b + 1]; ++m) {
            const int e = L.members[m];
            if (e < 0 || e >= k) return bad(LT_E_MEMBER_RANGE, b);
            if (kind[e] != kDistLintr) return bad(LT_E_MEMBER_KIND, b);
            if (N.blk[e] >= 0) return bad(LT_E_MEMBER_TWICE, b);
            if (!std::isfinite(L.constants[m])) return bad(LT_E_CONSTANT, b);
            N.blk[e] = b; N.row[e] = m; N.elem[m] = e; N.c[m] = L.constants[m];
        }
    for (int e = 0; e < k; ++e)
        if (kind[e] == kDistLintr && N.blk[e] < 0) return bad(LT_E_NO_BLOCK, e);
    // the matrix
    if (nb > 0 && L.row_ptr[0] != 0) return bad(LT_E_OFFSETS, 0);
    for (int b = 0; b < nb; ++b)
        for (int m = L.member_off[b]; m < L.member_off[b + 1]; ++m)
            if (L.row_ptr[m + 1] < L.row_ptr[m]) return bad(LT_E_OFFSETS, b);
    const int nnz = nb ? L.row_ptr[M] : 0;
    if (nnz > 0 && (!L.col || !L.val)) return bad(LT_E_NULL, -1);
    N.rptr.assign(L.row_ptr, L.row_ptr + (nb ? M + 1 : 0));
    if (!nb) N.rptr.assign(1, 0);
    N.col.resize(nnz); N.h.resize(nnz);
    for (int b = 0; b < nb; ++b) {
        const int l0 = L.latent_off[b], q = L.latent_off[b + 1] - l0;
        for (int m = L.member_off[b]; m < L.member_off[b + 1]; ++m)
            for (int p = L.row_ptr[m]; p < L.row_ptr[m + 1]; ++p) {
                const int l = L.col[p];
                if (l < 0 || l >= q || (p > L.row_ptr[m] && l <= L.col[p - 1])) return bad(LT_E_COLUMN, b);
                if (!std::isfinite(L.val[p])) return bad(LT_E_COEF, b);
                N.col[p] = l0 + l; N.h[p] = L.val[p];
            }
    }
    // the latents: twosd_set_distributions' reading of an element
    N.lkind.resize(Q); N.loff.assign(Q + 1, 0); N.lword.resize(Q);
    N.lp0.assign(Q, 0.0); N.lp1.assign(Q, 0.0); N.lvar.assign(Q, 0.0);
    long long ns = 0;
    for (int l = 0; l < Q; ++l) {
        if (L.latent_kind[l] < 0 || L.latent_kind[l] > 2) return bad(LT_E_LATENT_KIND, l);
        if (L.latent_kind[l] == 0) {
            if (L.latent_nsupport[l] < 1 || !L.latent_values || !L.latent_probs) return bad(LT_E_LATENT_SUPPORT, l);
            ns += L.latent_nsupport[l];
            if (ns > (long long)INT32_MAX) return bad(LT_E_TOO_LARGE, l);
        }
    }
    size_t at = 0;
    for (int l = 0; l < Q; ++l) {
        N.lkind[l] = L.latent_kind[l];
        N.lword[l] = k + l;
        if (N.lkind[l] == 0) {   // DISCRETE: sorted by value, values unique, probabilities >= 0
            const int n = L.latent_nsupport[l];
            std::vector<std::pair<double, double>> sp(n);
            for (int i = 0; i < n; ++i) sp[i] = {L.latent_values[at + i], L.latent_probs[at + i]};
            at += n;
            std::stable_sort(sp.begin(), sp.end(),
                             [](const std::pair<double, double> &a, const std::pair<double, double> &b) { return a.first < b.first; });
            double ps = 0.0, mu = 0.0, var = 0.0;
            for (int i = 0; i < n; ++i) {
                if (i && sp[i].first == sp[i - 1].first) return bad(LT_E_LATENT_SUPPORT, l);
                if (!(sp[i].second >= 0.0)) return bad(LT_E_LATENT_SUPPORT, l);
                N.lval.push_back(sp[i].first);
                N.lprob.push_back(sp[i].second);
                ps += sp[i].second; mu += sp[i].second * sp[i].first;
            }
            mu = ps > 0.0 ? mu / ps : 0.0;
            for (int i = 0; i < n; ++i) var += sp[i].second * (sp[i].first - mu) * (sp[i].first - mu);
            N.lvar[l] = ps > 0.0 ? var / ps : 0.0;
        } else if (N.lkind[l] == 1) {   // NORMAL(mean, variance)
            if (!(L.latent_param1[l] >= 0.0)) return bad(LT_E_LATENT_VARIANCE, l);
            N.lp0[l] = L.latent_param0[l];
            N.lp1[l] = std::sqrt(L.latent_param1[l]);
            N.lvar[l] = L.latent_param1[l];
        } else {                        // UNIFORM(left, right)
            N.lp0[l] = L.latent_param0[l];
            N.lp1[l] = L.latent_param1[l];
            const double w = L.latent_param1[l] - L.latent_param0[l];
            N.lvar[l] = w * w / 12.0;
        }
        N.loff[l + 1] = (int)N.lval.size();
    }
    T = std::move(N);
    return LT_OK;
}

// The selection key's scale of member row m: sqrt(2 / pi) sqrt(sum_l h^2 Var xi_l), the mean
// absolute deviation the row would have if it were normal.  A heuristic scale, not a bound.
inline double lintr_member_mad(const LintrTables &T, int m) {
    double var = 0.0;
    for (int p = T.rptr[m]; p < T.rptr[m + 1]; ++p) var += T.h[p] * T.h[p] * T.lvar[T.col[p]];
    return std::sqrt(2.0 / 3.14159265358979323846) * std::sqrt(var);
}

// Member row m at the latent values xi (Q): the contract's arithmetic, one rounding per product
// and per sum.  (The host restatement of lintr_apply_kernel; build without fp contraction.)
inline double lintr_member_value(const LintrTables &T, int m, const double *xi) {
    volatile double v = T.c[m];
    for (int p = T.rptr[m]; p < T.rptr[m + 1]; ++p) {
        volatile double t = T.h[p] * xi[T.col[p]];
        v = v + t;
    }
    return v;
}

#pragma GCC visibility pop
}  // namespace twosd
