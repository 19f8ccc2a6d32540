// Stand-alone host check of sqlp_amd/csrc/cut_i8.h (built with ASan + UBSan by
// tests/test_cut_i8_model.py; compile with -DTWOSD_CUT_I8_L=3 or 4).
//   cut_i8_check                 the limb range / reconstruction checks at the extremes
//   cut_i8_check in.bin out.bin  in: int32 k, nv, N; dmax[k], pc[nv k], dv[N k] (doubles).
//                                out: float t[N nv], double band[nv], int32 S[nv] -- the pass's score
//                                terms by the header's functions; exit 2 when a term leaves its band
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cut_i8.h"

using namespace twosd;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

static void check_value(double a, int E) {
    const int q = ci8::quantise(a, E);
    CHECK(std::abs(q) <= (1 << ci8::kQ));
    CHECK(std::fabs((double)q - std::ldexp(a, ci8::kQ - E)) <= 0.5);
    int8_t lb[ci8::kL];
    ci8::limbs(q, lb);
    long long back = 0;
    for (int l = 0; l < ci8::kL; ++l) {
        CHECK(lb[l] >= -64 && lb[l] <= 64);
        back = back * 128 + lb[l];
    }
    CHECK(back == q);
    if (E <= ci8::kQ + 1000) CHECK(ci8::quantise_by(a, std::ldexp(1.0, ci8::kQ - E)) == q);
}

static void extremes() {
    const int Es[] = {ci8::kEmin, -1, 0, 1, 20, 100};
    for (int E : Es) {
        const double sc = std::ldexp(1.0, E);
        const double vals[] = {sc, -sc, 0.0, -0.0, 4.9e-324, -4.9e-324, 2.2250738585072014e-308, std::nextafter(sc, 0.0),
                               -std::nextafter(sc, 0.0), sc / 3.0, -sc / 7.0, std::ldexp(sc, -ci8::kQ - 1), std::ldexp(sc, -ci8::kQ),
                               std::ldexp(1.5 * sc, -ci8::kQ), std::ldexp(sc, -1), std::ldexp(63.5 * sc, -7)};
        for (double a : vals) check_value(a, E);
        CHECK(ci8::scale_exp(sc) == E);
        CHECK(ci8::scale_exp(std::nextafter(sc, INFINITY)) == E + 1);
    }
    CHECK(ci8::scale_exp(0.0) == ci8::kEmin && ci8::scale_exp(4.9e-324) == ci8::kEmin);
    // every q in a window around each power of 128 and at the ends
    for (int q = -(1 << ci8::kQ); q <= (1 << ci8::kQ); q += (q > -70000 && q < 70000) ? 1 : 4099) {
        int8_t lb[ci8::kL];
        ci8::limbs(q, lb);
        long long back = 0;
        for (int l = 0; l < ci8::kL; ++l) {
            CHECK(lb[l] >= -64 && lb[l] <= 64);
            back = back * 128 + lb[l];
        }
        CHECK(back == q);
    }
}

template <typename T>
static bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    extremes();
    if (argc < 3) {
        std::printf("cut_i8 limbs %d: %d failures\n", ci8::kL, fails);
        return fails ? 1 : 0;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hd[3];
    if (!rd(f, hd, 3)) return 3;
    const int k = hd[0], nv = hd[1], N = hd[2];
    std::vector<double> dmax(k), pc((size_t)nv * k), dv((size_t)N * k);
    if (!rd(f, dmax.data(), dmax.size()) || !rd(f, pc.data(), pc.size()) || !rd(f, dv.data(), dv.size())) return 3;
    std::fclose(f);
    std::vector<int> E(k), S(nv);
    std::vector<int8_t> la((size_t)nv * k * ci8::kL), ld((size_t)N * k * ci8::kL);
    std::vector<double> band(nv);
    for (int e = 0; e < k; ++e) E[e] = ci8::scale_exp(dmax[e]);
    for (int v = 0; v < nv; ++v) {
        double um = 0.0;
        for (int e = 0; e < k; ++e) um = std::fmax(um, std::fabs(std::ldexp(pc[(size_t)v * k + e], E[e])));
        S[v] = ci8::scale_exp(um);
        double ns = 0.0;
        for (int e = 0; e < k; ++e) {
            ns += std::ldexp(dmax[e], -E[e]) + std::ldexp(std::fabs(pc[(size_t)v * k + e]), E[e] - S[v]);
            ci8::limbs(ci8::quantise(pc[(size_t)v * k + e], S[v] - E[e]), &la[((size_t)v * k + e) * ci8::kL]);
        }
        band[v] = ci8::band_term(k, S[v], ns);
    }
    for (int s = 0; s < N; ++s)
        for (int e = 0; e < k; ++e)
            ci8::limbs(ci8::quantise_by(dv[(size_t)s * k + e], std::ldexp(1.0, ci8::kQ - E[e])), &ld[((size_t)s * k + e) * ci8::kL]);
    std::vector<float> t((size_t)N * nv);
    int out_of_band = 0;
    for (int s = 0; s < N; ++s)
        for (int v = 0; v < nv; ++v) {
            int acc[ci8::kL] = {};
            long double exact = 0.0L;
            for (int e = 0; e < k; ++e) {
                const int8_t *a = &la[((size_t)v * k + e) * ci8::kL], *d = &ld[((size_t)s * k + e) * ci8::kL];
                for (int l1 = 0; l1 < ci8::kL; ++l1)
                    for (int l2 = 0; l1 + l2 < ci8::kL; ++l2) acc[l1 + l2] += (int)a[l1] * (int)d[l2];
                exact += (long double)pc[(size_t)v * k + e] * (long double)dv[(size_t)s * k + e];
            }
            for (int l = 0; l < ci8::kL; ++l) CHECK(std::abs(acc[l]) < (1 << 24));   // exact in fp32
            const float tv = ci8::combine(acc, std::ldexp(1.0f, S[v] + ci8::kOutShift));
            t[(size_t)s * nv + v] = tv;
            if (std::fabs((double)((long double)tv - exact)) > band[v]) ++out_of_band;
        }
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 3;
    std::fwrite(t.data(), sizeof(float), t.size(), o);
    std::fwrite(band.data(), sizeof(double), band.size(), o);
    std::vector<int32_t> S32(S.begin(), S.end());
    std::fwrite(S32.data(), sizeof(int32_t), S32.size(), o);
    std::fclose(o);
    std::printf("cut_i8 limbs %d: k %d nv %d N %d, %d out of band, %d failures\n", ci8::kL, k, nv, N, out_of_band, fails);
    return fails ? 1 : out_of_band ? 2 : 0;
}
