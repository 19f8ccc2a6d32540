// dist_tables_check.cpp -- sqlp_amd/csrc/dist_tables.h on the CPU (make sanitize_dist: host
// compiler, ASan + UBSan; driven by tests/test_dist_tables_host.py).
//   pick lines: for generated blocks, dist_pick over the built running sums against the literal
//     DISCRETE walk over the probabilities, at every running sum, its two fp64 neighbours, 0 and
//     1 - 2^-53;
//   error lines: every validation error on heap arrays of exactly the lengths the shapes give, so
//     a read past them stops the run;
//   table lines: the tables of a two-block layout with permuted, non-contiguous members.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>
#include "dist_tables.h"

using namespace twosd;

// the stream contract's walk, literally
static int walk(const std::vector<double> &p, double u) {
    const int R = (int)p.size();
    int i = 0;
    double cp = p[0];
    while (cp <= u && i < R - 1) cp = cp + p[++i];
    return i;
}

static uint64_t lcg(uint64_t &s) { return s = s * 6364136223846793005ull + 1442695040888963407ull; }
static double unit(uint64_t &s) { return (double)(lcg(s) >> 11) * 0x1p-53; }

// R probabilities of total mass `mass`; zeros: 0 none, 1 leading run, 2 trailing run, 3 runs inside
static std::vector<double> probabilities(int R, double mass, int zeros, uint64_t seed) {
    std::vector<double> p(R);
    double sum = 0.0;
    for (int r = 0; r < R; ++r) {
        p[r] = 0.05 + unit(seed);
        const bool zero = (zeros == 1 && r < (R + 2) / 3 && r < R - 1) || (zeros == 2 && r >= R - (R + 2) / 3 && r > 0) ||
                          (zeros == 3 && (r / 3) % 2 == 1);
        if (zero) p[r] = 0.0;
        sum += p[r];
    }
    for (int r = 0; r < R; ++r) p[r] = sum > 0.0 && mass > 0.0 ? p[r] * (mass / sum) : 0.0;
    return p;
}

static int check_pick(int R, double mass, int zeros) {
    const std::vector<double> p = probabilities(R, mass, zeros, 977u * R + 31u * zeros + (uint64_t)(mass * 16));
    const std::vector<int> kind(1, kDistBlock), moff{0, 1}, mem{0}, nreal{R};
    std::vector<double> val(R);
    for (int r = 0; r < R; ++r) val[r] = (double)r;
    DistTables T;
    int where = -1;
    const int rc = dist_tables_build(1, kind.data(), 1, moff.data(), mem.data(), nreal.data(), p.data(), val.data(), T, &where);
    if (rc != DT_OK) { printf("pick R=%d mass=%g zeros=%d : build failed %d\n", R, mass, zeros, rc); return 1; }
    std::vector<double> probes{0.0, 1.0 - 0x1p-53};
    for (int r = 0; r < R; ++r) {
        const double c = T.cum[r];
        probes.push_back(c);
        probes.push_back(std::nextafter(c, -std::numeric_limits<double>::infinity()));
        probes.push_back(std::nextafter(c, std::numeric_limits<double>::infinity()));
    }
    int bad = 0, ties = 0;
    for (int r = 1; r < R; ++r) {
        ties += T.cum[r] == T.cum[r - 1];
        if (T.cum[r] < T.cum[r - 1]) ++bad;   // nondecreasing
    }
    for (double u : probes) {
        if (u < 0.0) continue;   // the lower neighbour of a running sum 0: no uniform is negative
        const int a = dist_pick(T.cum.data(), R, u), b = walk(p, u);
        if (a != b) {
            if (!bad) printf("  mismatch R=%d u=%.17g pick=%d walk=%d\n", R, u, a, b);
            ++bad;
        }
    }
    printf("pick R=%d mass=%g zeros=%d : probes=%zu ties=%d last=%.17g mismatches=%d\n", R, mass, zeros, probes.size(), ties,
           T.cum[R - 1], bad);
    return bad;
}

// one validation case: exact-length heap copies of the arrays, the expected code
struct Case {
    const char *name;
    int expect;
    std::vector<int> kind, moff, mem, nreal;
    std::vector<double> p, v;
};

static int check_error(const Case &c) {
    const int k = (int)c.kind.size(), nb = (int)c.nreal.size();
    // exactly-sized copies (a vector's capacity may exceed its size)
    int *kind = new int[c.kind.size()], *moff = new int[c.moff.size()], *mem = new int[c.mem.size()], *nreal = new int[c.nreal.size()];
    double *p = new double[c.p.size()], *v = new double[c.v.size()];
    for (size_t i = 0; i < c.kind.size(); ++i) kind[i] = c.kind[i];
    for (size_t i = 0; i < c.moff.size(); ++i) moff[i] = c.moff[i];
    for (size_t i = 0; i < c.mem.size(); ++i) mem[i] = c.mem[i];
    for (size_t i = 0; i < c.nreal.size(); ++i) nreal[i] = c.nreal[i];
    for (size_t i = 0; i < c.p.size(); ++i) p[i] = c.p[i];
    for (size_t i = 0; i < c.v.size(); ++i) v[i] = c.v[i];
    DistTables T;
    T.lead.assign(1, 77);   // untouched on an error
    int where = -1;
    const int rc = dist_tables_build(k, kind, nb, moff, mem, nreal, p, v, T, &where);
    const bool kept = rc == DT_OK || (T.lead.size() == 1 && T.lead[0] == 77);
    printf("error %s : code=%d expect=%d where=%d kept=%d (%s)\n", c.name, rc, c.expect, where, (int)kept, dist_err_text(rc));
    delete[] kind; delete[] moff; delete[] mem; delete[] nreal; delete[] p; delete[] v;
    return rc != c.expect || !kept;
}

int main() {
    int bad = 0;
    for (int R : {1, 2, 3, 7, 1000})
        for (double mass : {1.0, 0.9, 0.0})
            for (int zeros : {0, 1, 2, 3}) bad += check_pick(R, mass, zeros);

    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int B = kDistBlock;
    // k = 4 elements: 0 DISCRETE, 1..3 block members unless stated; one block [2, 1] with R = 2
    const std::vector<Case> cases = {
        {"ok", DT_OK, {0, B, B, 1}, {0, 2}, {2, 1}, {2}, {0.5, 0.5}, {1, 2, 3, 4}},
        {"no_blocks", DT_OK, {0, 1, 2, 0}, {}, {}, {}, {}, {}},
        {"member_off_start", DT_E_OFFSETS, {0, B, B, 1}, {1, 2}, {2, 1}, {2}, {0.5, 0.5}, {1, 2, 3, 4}},
        {"empty_block", DT_E_EMPTY_BLOCK, {0, B, B, 1}, {0, 2, 2}, {2, 1}, {2, 1}, {0.5, 0.5, 1.0}, {1, 2, 3, 4}},
        {"nreal_zero", DT_E_NREAL, {0, B, B, 1}, {0, 2}, {2, 1}, {0}, {}, {}},
        {"nreal_negative", DT_E_NREAL, {0, B, B, 1}, {0, 2}, {2, 1}, {-3}, {}, {}},
        {"too_large", DT_E_TOO_LARGE, {0, B, B, 1}, {0, 2}, {2, 1}, {INT32_MAX}, {}, {}},
        {"member_low", DT_E_MEMBER_RANGE, {0, B, B, 1}, {0, 2}, {2, -1}, {2}, {0.5, 0.5}, {1, 2, 3, 4}},
        {"member_high", DT_E_MEMBER_RANGE, {0, B, B, 1}, {0, 2}, {4, 1}, {2}, {0.5, 0.5}, {1, 2, 3, 4}},
        {"member_kind", DT_E_MEMBER_KIND, {0, B, B, 1}, {0, 2}, {2, 0}, {2}, {0.5, 0.5}, {1, 2, 3, 4}},
        {"twice_in_one", DT_E_MEMBER_TWICE, {0, B, B, 1}, {0, 2}, {2, 2}, {2}, {0.5, 0.5}, {1, 2, 3, 4}},
        {"in_two_blocks", DT_E_MEMBER_TWICE, {0, B, B, 1}, {0, 2, 3}, {2, 1, 2}, {1, 1}, {1.0, 1.0}, {1, 2, 3}},
        {"in_no_block", DT_E_NO_BLOCK, {0, B, B, B}, {0, 2}, {2, 1}, {2}, {0.5, 0.5}, {1, 2, 3, 4}},
        {"kind3_without_blocks", DT_E_NO_BLOCK, {0, B}, {}, {}, {}, {}, {}},
        {"prob_negative", DT_E_PROB, {0, B, B, 1}, {0, 2}, {2, 1}, {2}, {0.5, -0.5}, {1, 2, 3, 4}},
        {"prob_nan", DT_E_PROB, {0, B, B, 1}, {0, 2}, {2, 1}, {2}, {nan, 0.5}, {1, 2, 3, 4}},
        {"prob_inf", DT_E_PROB, {0, B, B, 1}, {0, 2}, {2, 1}, {2}, {0.5, inf}, {1, 2, 3, 4}},
        {"value_nan", DT_E_VALUE, {0, B, B, 1}, {0, 2}, {2, 1}, {2}, {0.5, 0.5}, {1, 2, nan, 4}},
        {"value_inf", DT_E_VALUE, {0, B, B, 1}, {0, 2}, {2, 1}, {2}, {0.5, 0.5}, {1, 2, 3, -inf}},
    };
    for (const Case &c : cases) bad += check_error(c);
    {   // NULL arrays
        DistTables T;
        const int kind[1] = {0};
        const int a = dist_tables_build(1, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, T, nullptr);
        const int b = dist_tables_build(1, kind, 1, nullptr, nullptr, nullptr, nullptr, nullptr, T, nullptr);
        const int c = dist_tables_build(0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, T, nullptr);
        printf("error null : kind=%d blocks=%d empty=%d\n", a, b, c);
        bad += a != DT_E_NULL || b != DT_E_NULL || c != DT_OK;
    }
    {   // k = 7: block 0 = [4, 1, 6] (R = 2), block 1 = [0] (R = 3); elements 2, 3, 5 independent
        const std::vector<int> kind{B, B, 0, 1, B, 2, B}, moff{0, 3, 4}, mem{4, 1, 6, 0}, nreal{2, 3};
        const std::vector<double> p{0.25, 0.5, 0.0, 0.1, 0.2}, v{10, 11, 12, 20, 21, 22, 1, 2, 3};
        DistTables T;
        int where = -1;
        const int rc = dist_tables_build(7, kind.data(), 2, moff.data(), mem.data(), nreal.data(), p.data(), v.data(), T, &where);
        printf("table rc=%d lead=", rc);
        for (int x : T.lead) printf("%d,", x);
        printf(" blk=");
        for (int x : T.blk) printf("%d,", x);
        printf(" col=");
        for (int x : T.col) printf("%d,", x);
        printf(" blocks=");
        for (const DistBlock &b : T.block) printf("(%d,%d,%d,%d)", b.R, b.n, b.poff, b.voff);
        printf(" cum=");
        for (double x : T.cum) printf("%.17g,", x);
        printf(" mad=%.17g,%.17g\n", dist_member_mad(T, 0, 1), dist_member_mad(T, 1, 0));
        bad += rc != DT_OK;
    }
    printf("%s\n", bad ? "FAILED" : "all ok");
    return bad ? 1 : 0;
}
