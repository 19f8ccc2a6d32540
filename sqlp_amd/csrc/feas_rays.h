// feas_rays.h -- the pure arithmetic of feasibility rays: normalisation, the
// snap, the dedup key and the feasibility row of a (ray, scenario) pair.  Host and device, no HIP
// include: feas.hip uses it in its kernels and in twosd_fray_key, tests/native/feas_rays_check.cpp
// drives it alone under the host compiler's sanitizers.
//
// A ray sigma (mv doubles) has the sign convention of a dual: sigma_i >= 0 on G rows, <= 0 on L
// rows (bound rows are L), free on E rows; sigma' W_j <= 0 for every structural column; sigma' b > 0
// certifies that the LP with right-hand side b has no solution.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FR_HD __host__ __device__
#else
#define FR_HD
#endif

namespace twosd {
namespace fr {

// splitmix64 finalizer: the mix64 of twosd_internal.h / dvs_keys.h (restated: this header includes neither)
FR_HD inline uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

FR_HD inline uint64_t bits_of(double v) {
    union { double d; uint64_t u; } x;
    x.d = v;
    return x.u;
}

// max |sigma_i|; NaN if any component is not finite
FR_HD inline double max_abs(const double *sigma, int mv) {
    double mx = 0.0;
    for (int i = 0; i < mv; ++i) {
        if (!isfinite(sigma[i])) return NAN;
        const double a = fabs(sigma[i]);
        mx = a > mx ? a : mx;
    }
    return mx;
}

// |sigma_i| <= zero_rel (1 + max |sigma|) -> 0, as the LP kernel snaps a recovered pi (HPI_ZERO)
FR_HD inline void snap(double *sigma, int mv, double zero_rel) {
    const double mx = max_abs(sigma, mv);
    if (!(mx >= 0.0)) return;
    const double zt = zero_rel * (1.0 + mx);
    for (int i = 0; i < mv; ++i)
        if (fabs(sigma[i]) <= zt) sigma[i] = 0.0;
}

// out = sigma / max |sigma_i| (in place allowed); false (out untouched) for an all-zero ray or one
// with a component that is not finite.  A zero keeps the sign +0.
FR_HD inline bool normalise(const double *sigma, int mv, double *out) {
    const double mx = max_abs(sigma, mv);
    if (!(mx > 0.0)) return false;
    for (int i = 0; i < mv; ++i) {
        const double v = sigma[i] / mx;
        out[i] = v == 0.0 ? 0.0 : v;
    }
    return true;
}

// Key of a normalised ray: the components rounded to 24 significant bits (sign, exponent and 23
// mantissa bits, round half up on the magnitude: the rounding of the LP kernel's dual key) next to
// their row, mixed and summed.  Zeros of either sign give the same word.
FR_HD inline uint64_t key(const double *nrm, int mv) {
    uint64_t h = 0;
    for (int i = 0; i < mv; ++i) {
        const double v = nrm[i] == 0.0 ? 0.0 : nrm[i];
        const uint64_t b = (bits_of(v) + (1ull << 28)) >> 29;
        h += mix64(((uint64_t)i << 35) | b);
    }
    return h;
}

// The feasibility row alpha + beta' x <= 0 of (sigma, scenario): rb = [r_w - W s ; hi - lo] is the
// scenario's right-hand side at x = 0 (mv), T its dense technology matrix (mv x n1, row-major; the
// bound rows are zero).  alpha = sum_i sigma_i rb_i and beta_j = -sum_i T_ij sigma_i, both in index
// order with every product and every sum rounded on its own (compile with -ffp-contract=off).
FR_HD inline void row(const double *sigma, int mv, const double *rb, const double *T, int n1, double *alpha, double *beta) {
    double a = 0.0;
    for (int i = 0; i < mv; ++i) {
        const double p = sigma[i] * rb[i];
        a = a + p;
    }
    *alpha = a;
    for (int j = 0; j < n1; ++j) {
        double c = 0.0;
        for (int i = 0; i < mv; ++i) {
            const double p = T[(size_t)i * n1 + j] * sigma[i];
            c = c + p;
        }
        beta[j] = -c;
    }
}

}  // namespace fr
}  // namespace twosd
