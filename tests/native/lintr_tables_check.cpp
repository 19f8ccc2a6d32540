// lintr_tables_check.cpp -- the LINTR tables of sqlp_amd/csrc/lintr_tables.h on the CPU, built
// with ASan + UBSan by `make sanitize_lintr` and run directly (tests/test_lintr_tables_host.py).
// Every array handed to lintr_tables_build is a heap vector of exactly the length the shapes give,
// so a read past the contract is an ASan report.  Prints one line per case; "all ok" last.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>
#include "lintr_tables.h"

using namespace twosd;

// k = 7.  Block 0: members [5, 0, 3] (non-contiguous, not ascending), q = 2 (DISCRETE with an
// unsorted support, UNIFORM), rows with 2, 1 and 0 entries.  Block 1: members [6, 4] (descending),
// q = 3 (NORMAL x 2, DISCRETE), rows with q = 3 and 1 entries.
struct Case {
    int k = 7;
    std::vector<int> kind{4, 1, 0, 4, 4, 4, 4};
    int nblocks = 2;
    std::vector<int> member_off{0, 3, 5}, members{5, 0, 3, 6, 4};
    std::vector<double> constants{10.0, -2.0, 0.5, 1.0, 2.0};
    std::vector<int> latent_off{0, 2, 5}, latent_kind{0, 2, 1, 1, 0}, latent_nsupport{3, 0, 0, 0, 2};
    std::vector<double> latent_values{2.0, -1.0, 0.0, 1.0, 3.0}, latent_probs{0.25, 0.5, 0.25, 0.5, 0.5};
    std::vector<double> latent_param0{0.0, -1.0, 0.0, 5.0, 0.0}, latent_param1{0.0, 3.0, 1.0, 4.0, 0.0};
    std::vector<int> row_ptr{0, 2, 3, 3, 6, 7}, col{0, 1, 1, 0, 1, 2, 1};
    std::vector<double> val{1.5, -0.5, 2.0, 1.0, 0.0, -3.0, 0.25};
    LintrSpec spec() const {
        return LintrSpec{nblocks, member_off.data(), members.data(), constants.data(), latent_off.data(), latent_kind.data(),
                         latent_nsupport.data(), latent_values.data(), latent_probs.data(), latent_param0.data(),
                         latent_param1.data(), row_ptr.data(), col.data(), val.data()};
    }
};

static int failures = 0;

static void expect(const char *name, const Case &c, int code, int where_want) {
    LintrTables T;
    T.M = -7;                                  // a sentinel: a refused build must not write T
    int where = -99;
    const int rc = lintr_tables_build(c.k, c.kind.data(), c.spec(), T, &where);
    const int kept = rc == LT_OK ? 1 : (T.M == -7 && T.elem.empty());
    printf("error %s : code=%d where=%d kept=%d text=\"%s\"\n", name, rc, where, kept, lintr_err_text(rc));
    if (rc != code || (where_want > -50 && where != where_want) || !kept) {
        printf("  FAILED: expected code %d where %d\n", code, where_want);
        ++failures;
    }
}

template <typename T>
static std::string join(const std::vector<T> &v) {
    std::string s;
    for (const T &x : v) {
        char buf[40];
        snprintf(buf, sizeof buf, "%.17g,", (double)x);
        s += buf;
    }
    return s;
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const Case good;
    // ---- the tables of the good case
    {
        LintrTables T;
        int where = -1;
        const int rc = lintr_tables_build(good.k, good.kind.data(), good.spec(), T, &where);
        printf("table rc=%d M=%d Q=%d blk=%s row=%s elem=%s c=%s rptr=%s col=%s h=%s\n", rc, T.M, T.Q, join(T.blk).c_str(),
               join(T.row).c_str(), join(T.elem).c_str(), join(T.c).c_str(), join(T.rptr).c_str(), join(T.col).c_str(), join(T.h).c_str());
        printf("latents kind=%s off=%s word=%s val=%s prob=%s p0=%s p1=%s var=%s\n", join(T.lkind).c_str(), join(T.loff).c_str(),
               join(T.lword).c_str(), join(T.lval).c_str(), join(T.lprob).c_str(), join(T.lp0).c_str(), join(T.lp1).c_str(),
               join(T.lvar).c_str());
        if (rc != LT_OK) { ++failures; printf("  FAILED: the good case was refused\n"); }
        else {
            std::vector<double> mad, value;
            const std::vector<double> xi{2.0, 0.5, -1.25, 3.0, 1.0};
            for (int m = 0; m < T.M; ++m) { mad.push_back(lintr_member_mad(T, m)); value.push_back(lintr_member_value(T, m, xi.data())); }
            printf("members mad=%s value=%s\n", join(mad).c_str(), join(value).c_str());
        }
    }
    // ---- no LINTR blocks: nothing is read, empty tables
    {
        Case c;
        c.kind = {0, 1, 0, 2, 1, 0, 2};
        c.nblocks = 0;
        LintrTables T;
        int where = -1;
        const LintrSpec none{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        const int rc = lintr_tables_build(c.k, c.kind.data(), none, T, &where);
        printf("empty rc=%d M=%d Q=%d rptr=%s\n", rc, T.M, T.Q, join(T.rptr).c_str());
        if (rc != LT_OK || T.M || T.Q) ++failures;
    }
    // ---- every refusal, on exactly-sized arrays
    expect("ok", good, LT_OK, -99);
    { Case c; c.kind[1] = 4; expect("in_no_block", c, LT_E_NO_BLOCK, 1); }
    { Case c; c.nblocks = 0; expect("kind4_without_blocks", c, LT_E_NO_BLOCK, 0); }
    { Case c; c.members[3] = 0; expect("in_two_blocks", c, LT_E_MEMBER_TWICE, 1); }
    { Case c; c.members[2] = 5; expect("twice_in_one", c, LT_E_MEMBER_TWICE, 0); }
    { Case c; c.members[1] = 1; expect("member_kind", c, LT_E_MEMBER_KIND, 0); }
    { Case c; c.members[4] = -1; expect("member_low", c, LT_E_MEMBER_RANGE, 1); }
    { Case c; c.members[4] = 7; expect("member_high", c, LT_E_MEMBER_RANGE, 1); }
    { Case c; c.member_off = {0, 3, 3}; expect("empty_block", c, LT_E_EMPTY_BLOCK, 1); }
    { Case c; c.member_off = {1, 3, 5}; expect("member_off_start", c, LT_E_OFFSETS, 0); }
    { Case c; c.latent_off = {0, 2, 2}; expect("no_latent", c, LT_E_NLATENT, 1); }
    { Case c; c.latent_off = {0, 0, 5}; expect("no_latent_first", c, LT_E_NLATENT, 0); }
    { Case c; c.row_ptr = {1, 2, 3, 3, 6, 7}; expect("row_ptr_start", c, LT_E_OFFSETS, 0); }
    { Case c; c.row_ptr = {0, 2, 1, 3, 6, 7}; expect("row_ptr_decreases", c, LT_E_OFFSETS, 0); }
    { Case c; c.col[0] = -1; expect("column_low", c, LT_E_COLUMN, 0); }
    { Case c; c.col[1] = 2; expect("column_high", c, LT_E_COLUMN, 0); }
    { Case c; c.col[5] = 3; expect("column_high_second_block", c, LT_E_COLUMN, 1); }
    { Case c; c.col[4] = 0; expect("column_repeated", c, LT_E_COLUMN, 1); }
    { Case c; c.col[3] = 2; c.col[5] = 0; expect("column_descending", c, LT_E_COLUMN, 1); }
    { Case c; c.constants[3] = nan; expect("constant_nan", c, LT_E_CONSTANT, 1); }
    { Case c; c.constants[0] = -inf; expect("constant_inf", c, LT_E_CONSTANT, 0); }
    { Case c; c.val[2] = nan; expect("coef_nan", c, LT_E_COEF, 0); }
    { Case c; c.val[6] = inf; expect("coef_inf", c, LT_E_COEF, 1); }
    { Case c; c.latent_kind[1] = 3; expect("latent_kind", c, LT_E_LATENT_KIND, 1); }
    { Case c; c.latent_kind[2] = -1; expect("latent_kind_negative", c, LT_E_LATENT_KIND, 2); }
    { Case c; c.latent_nsupport[0] = 0; c.latent_values = {1.0, 3.0}; c.latent_probs = {0.5, 0.5}; expect("latent_support_empty", c, LT_E_LATENT_SUPPORT, 0); }
    { Case c; c.latent_values[2] = 2.0; expect("latent_support_repeated", c, LT_E_LATENT_SUPPORT, 0); }
    { Case c; c.latent_probs[4] = -0.5; expect("latent_prob_negative", c, LT_E_LATENT_SUPPORT, 4); }
    { Case c; c.latent_probs[1] = nan; expect("latent_prob_nan", c, LT_E_LATENT_SUPPORT, 0); }
    { Case c; c.latent_param1[3] = -4.0; expect("latent_variance_negative", c, LT_E_LATENT_VARIANCE, 3); }
    { Case c; c.latent_param1[2] = nan; expect("latent_variance_nan", c, LT_E_LATENT_VARIANCE, 2); }
    // the size guard, from the shapes alone: the arrays of Q entries are one element long and never read
    {
        Case c;
        c.latent_off = {0, 2, 2147483647 - 6};     // k + Q = 7 + (2^31 - 7) = 2^31: the first sum that is refused
        c.latent_kind = {0}; c.latent_nsupport = {0}; c.latent_param0 = {0.0}; c.latent_param1 = {0.0};
        expect("too_large", c, LT_E_TOO_LARGE, 1);
    }
    // NULL arrays
    {
        Case c;
        LintrTables T;
        int where = 0;
        LintrSpec s = c.spec();
        s.constants = nullptr;
        const int a = lintr_tables_build(c.k, c.kind.data(), s, T, &where);
        const int b = lintr_tables_build(c.k, nullptr, c.spec(), T, &where);
        s = c.spec();
        s.val = nullptr;
        const int d = lintr_tables_build(c.k, c.kind.data(), s, T, &where);
        printf("error null : constants=%d kind=%d val=%d empty=%d\n", a, b, d, (int)T.elem.empty());
        if (a != LT_E_NULL || b != LT_E_NULL || d != LT_E_NULL || !T.elem.empty()) ++failures;
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("all ok\n");
    return 0;
}
