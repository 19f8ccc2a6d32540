// feas_rays_check.cpp -- drives sqlp_amd/csrc/feas_rays.h alone on the host (make sanitize_feas: host
// compiler, -fsanitize=address,undefined, -ffp-contract=off) and prints, for a table of cases, the
// normalised ray, its key and a feasibility row on exactly-sized arrays; tests/test_feas_rays_host.py
// compares the output with numpy.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "feas_rays.h"

using namespace twosd;

static void print_vec(const char *tag, const std::vector<double> &v) {
    printf("%s", tag);
    for (double x : v) printf(" %a", x);
    printf("\n");
}

static void run_case(const char *name, const std::vector<double> &sigma, const std::vector<double> &rb, const std::vector<double> &T,
                     int n1) {
    const int mv = (int)sigma.size();
    printf("case %s mv %d n1 %d\n", name, mv, n1);
    print_vec("sigma", sigma);
    std::vector<double> s(sigma);   // exactly mv entries: an access past the end is the sanitizer's to report
    fr::snap(s.data(), mv, 1e-12);
    print_vec("snapped", s);
    std::vector<double> nrm(mv);
    const bool ok = fr::normalise(s.data(), mv, nrm.data());
    printf("ok %d\n", ok ? 1 : 0);
    if (!ok) return;
    print_vec("normalised", nrm);
    printf("key %" PRIu64 "\n", fr::key(nrm.data(), mv));
    if (!rb.empty()) {
        print_vec("rb", rb);
        print_vec("T", T);
        double alpha = 0.0;
        std::vector<double> beta(n1 > 0 ? n1 : 1);
        fr::row(nrm.data(), mv, rb.data(), T.data(), n1, &alpha, beta.data());
        beta.resize(n1);
        printf("alpha %a\n", alpha);
        print_vec("beta", beta);
    }
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    run_case("unit", {1.0}, {2.0}, {3.0}, 1);
    run_case("signs", {0.5, -2.0, 0.0, 1.5, -0.25}, {1.0, 2.0, 3.0, -4.0, 0.1},
             {1.0, 0.0, -1.0, 0.5, 0.25, 2.0, 0.0, 0.0, 3.0, -3.0, 1e-3, 7.0, -1.0, 1.0, 0.0}, 3);
    run_case("scaled", {1.5, -6.0, 0.0, 4.5, -0.75}, {}, {}, 0);            // 3 x "signs": the same normalised ray and key
    run_case("flipped", {0.5, -2.0, 0.0, -1.5, -0.25}, {}, {}, 0);
    run_case("tiny", {1.0, 1e-13, -2e-12, 3e-12, -1.0}, {}, {}, 0);         // entries at the snap threshold 1e-12 (1 + 1)
    run_case("perturbed", {0.5, -2.0, 0.0, 1.5 * (1.0 + 1e-9), -0.25}, {}, {}, 0);   // below the 24-bit rounding: the key of "signs"
    run_case("thirds", {1.0 / 3.0, -2.0 / 3.0, 1.0 / 7.0, 0.1, -0.3}, {0.1, 0.2, 0.3, 0.4, 0.5},
             {0.1, 0.7, 0.2, 0.3, 0.9, 0.11, 0.13, 0.17, 0.19, 0.23}, 2);
    run_case("negzero", {-0.0, 2.0, 0.0}, {}, {}, 0);
    run_case("zero", {0.0, 0.0, -0.0}, {}, {}, 0);
    run_case("nan", {1.0, nan, 0.5}, {}, {}, 0);
    run_case("inf", {1.0, -inf, 0.5}, {}, {}, 0);
    run_case("n1zero", {2.0, -4.0}, {1.0, 1.0}, {}, 0);
    return 0;
}
