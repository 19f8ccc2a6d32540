// dist_tables.h -- joint discrete distributions ("blocks") of the scenario
// sampler: the tables a set of blocks becomes, their validation, and the pick of a realisation at
// a uniform.  No HIP in here: api.hip builds the tables, the kernels of sampler.hip call the same
// dist_pick, and tests/native/dist_tables_check.cpp includes this file alone and checks both on
// the CPU.
//
// A block is an ordered member list e_0 .. e_{n-1} (indices into the random-element layout, in the
// caller's order; e_0 is the block's lead) and R realisations in the caller's order, realisation r
// with probability p_r >= 0 and one value per member, V[r][j].  Nothing is sorted, merged or
// normalised.  At a uniform u the realisation is the DISCRETE walk over p:
//     i = 0, cp = p_0; while (cp <= u && i < R - 1) cp = cp + p_{++i}
// The tables hold the walk's successive cp (cum, the same sequential fp64 additions), so the
// walk's index is the first i with cum[i] > u, else R - 1, and a binary search finds it: cum is
// nondecreasing because every p_r >= 0 and a rounded sum of a nonnegative term never decreases.
#pragma once
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#ifdef __HIPCC__
#define TWOSD_DT_HD __host__ __device__ __forceinline__
#else
#define TWOSD_DT_HD static inline
#endif

namespace twosd {
#pragma GCC visibility push(hidden)

constexpr int kDistBlock = 3;   // kind of a block member (TWOSD_DIST_BLOCK)

// what dist_tables_build returns; *where is the block (DT_E_OFFSETS .. DT_E_VALUE) or the element
// (DT_E_NO_BLOCK) it is about
enum DistErr : int {
    DT_OK = 0,
    DT_E_NULL,           // a needed array is NULL, k < 0 or nblocks < 0
    DT_E_OFFSETS,        // member_off[0] != 0
    DT_E_EMPTY_BLOCK,    // a block without members (member_off not increasing)
    DT_E_NREAL,          // nreal < 1
    DT_E_TOO_LARGE,      // a table past 2^31 - 1 entries (offsets are 32-bit)
    DT_E_MEMBER_RANGE,   // a member index outside [0, k)
    DT_E_MEMBER_KIND,    // a member whose kind is not kDistBlock
    DT_E_MEMBER_TWICE,   // an element in two blocks, or twice in one
    DT_E_NO_BLOCK,       // an element of kind kDistBlock that is in no block
    DT_E_PROB,           // a negative or non-finite probability
    DT_E_VALUE           // a non-finite value
};

inline const char *dist_err_text(int err) {
    switch (err) {
    case DT_OK: return "ok";
    case DT_E_NULL: return "NULL argument or negative count";
    case DT_E_OFFSETS: return "member_off[0] is not 0";
    case DT_E_EMPTY_BLOCK: return "block without members";
    case DT_E_NREAL: return "block with nreal < 1";
    case DT_E_TOO_LARGE: return "tables past 2^31 - 1 entries";
    case DT_E_MEMBER_RANGE: return "member index outside [0, k)";
    case DT_E_MEMBER_KIND: return "member whose kind is not 3 (block member)";
    case DT_E_MEMBER_TWICE: return "element in two blocks or twice in one";
    case DT_E_NO_BLOCK: return "element of kind 3 (block member) in no block";
    case DT_E_PROB: return "negative or non-finite probability";
    case DT_E_VALUE: return "non-finite value";
    }
    return "unknown error";
}

struct DistBlock {
    int R, n;            // realisations, members
    int poff, voff;      // its first entry of cum / prob, and of val
};

struct DistTables {
    std::vector<int> lead, blk, col;   // k: lead element (e itself outside a block), block (-1), member column j
    std::vector<DistBlock> block;
    std::vector<double> prob, cum;     // sum R: p_r as given; the walk's running sums
    std::vector<double> val;           // per block [R][n], realisation-major: members that are neighbours in
                                       //   the layout are neighbouring doubles of one realisation
};

// The realisation of a block at u: the first i with cum[i] > u, else R - 1 (R >= 1).
TWOSD_DT_HD int dist_pick(const double *cum, int R, double u) {
    int lo = 0, hi = R - 1;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cum[mid] > u) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// Checks the caller's blocks against kind[k] and builds the tables.  The shapes are checked before
// any of members / probs / values is read, and those are read only inside the lengths the shapes
// give: member_off[nblocks], sum nreal, sum nreal * n.  T is written on DT_OK only.
inline int dist_tables_build(int k, const int *kind, int nblocks, const int *member_off, const int *members, const int *nreal,
                             const double *probs, const double *values, DistTables &T, int *where) {
    const auto bad = [&](int code, int w) { if (where) *where = w; return code; };
    if (k < 0 || nblocks < 0 || (k > 0 && !kind)) return bad(DT_E_NULL, -1);
    if (nblocks > 0 && (!member_off || !members || !nreal || !probs || !values)) return bad(DT_E_NULL, -1);
    DistTables N;
    N.lead.resize(k); N.blk.assign(k, -1); N.col.assign(k, 0);
    for (int e = 0; e < k; ++e) N.lead[e] = e;
    if (nblocks > 0 && member_off[0] != 0) return bad(DT_E_OFFSETS, 0);
    long long np = 0, nv = 0;
    for (int b = 0; b < nblocks; ++b) {
        const long long n = (long long)member_off[b + 1] - member_off[b];
        if (n < 1) return bad(DT_E_EMPTY_BLOCK, b);
        if (nreal[b] < 1) return bad(DT_E_NREAL, b);
        N.block.push_back(DistBlock{nreal[b], (int)n, (int)np, (int)nv});
        np += nreal[b];
        nv += (long long)nreal[b] * n;
        if (np > INT32_MAX || nv > INT32_MAX) return bad(DT_E_TOO_LARGE, b);
    }
    for (int b = 0; b < nblocks; ++b)
        for (int j = 0; j < N.block[b].n; ++j) {
            const int e = members[member_off[b] + j];
            if (e < 0 || e >= k) return bad(DT_E_MEMBER_RANGE, b);
            if (kind[e] != kDistBlock) return bad(DT_E_MEMBER_KIND, b);
            if (N.blk[e] >= 0) return bad(DT_E_MEMBER_TWICE, b);
            N.blk[e] = b; N.col[e] = j; N.lead[e] = members[member_off[b]];
        }
    for (int e = 0; e < k; ++e)
        if (kind[e] == kDistBlock && N.blk[e] < 0) return bad(DT_E_NO_BLOCK, e);
    N.prob.resize((size_t)np); N.cum.resize((size_t)np); N.val.resize((size_t)nv);
    for (int b = 0; b < nblocks; ++b) {
        const DistBlock &B = N.block[b];
        double cp = 0.0;
        for (int r = 0; r < B.R; ++r) {
            const double p = probs[B.poff + r];
            if (!(p >= 0.0) || !std::isfinite(p)) return bad(DT_E_PROB, b);
            cp = r ? cp + p : p;   // the walk's cp: p_0, then one rounded addition per step
            N.prob[B.poff + r] = p;
            N.cum[B.poff + r] = cp;
        }
        for (long long i = 0; i < (long long)B.R * B.n; ++i) {
            if (!std::isfinite(values[B.voff + i])) return bad(DT_E_VALUE, b);
            N.val[B.voff + i] = values[B.voff + i];
        }
    }
    T = std::move(N);
    return DT_OK;
}

// Mean absolute deviation E|V - E V| of member column j of block b under p / sum p (0 when sum p
// is 0): the DISCRETE formula of twosd_set_distributions over the realisations.
inline double dist_member_mad(const DistTables &T, int b, int j) {
    const DistBlock &B = T.block[b];
    double ps = 0.0, mu = 0.0, mad = 0.0;
    for (int r = 0; r < B.R; ++r) { mu += T.prob[B.poff + r] * T.val[B.voff + (size_t)r * B.n + j]; ps += T.prob[B.poff + r]; }
    mu = ps > 0.0 ? mu / ps : 0.0;
    for (int r = 0; r < B.R; ++r) mad += T.prob[B.poff + r] * std::fabs(T.val[B.voff + (size_t)r * B.n + j] - mu);
    return ps > 0.0 ? mad / ps : 0.0;
}

#pragma GCC visibility pop
}  // namespace twosd
