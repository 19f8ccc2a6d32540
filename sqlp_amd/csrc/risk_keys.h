// risk_keys.h -- the host-checkable arithmetic of the quantile selection (risk.hip): the
// order-preserving 64-bit key of an fp64 value and the exact threshold t = ceil(level Q).
// No HIP: tests/native/risk_check.cpp compiles it with the host compiler under ASan + UBSan.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define RISK_HD __host__ __device__
#else
#define RISK_HD
#endif

namespace twosd {

// The sign-flip map: a negative value's bits are complemented, any other value gets its sign bit
// set, so unsigned order of the keys is the numeric order of the values with -0 before +0 (and
// NaNs at the two ends by sign, deterministic but meaningless).
RISK_HD inline uint64_t risk_key(double v) {
    uint64_t b;
    memcpy(&b, &v, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

RISK_HD inline double risk_unkey(uint64_t key) {
    const uint64_t b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
    double v;
    memcpy(&v, &b, sizeof v);
    return v;
}

// t = ceil(level * Q), exactly.  A double in (0, 1) is m 2^-sh with an integer m < 2^53 and
// sh >= 53, so level * Q = (m Q) / 2^sh with m Q < 2^117: one 128-bit product, a shift and the
// test of the bits shifted out.  1 <= t <= Q for Q >= 1.
inline uint64_t risk_threshold(double level, uint64_t Q) {
    int e = 0;
    const double f = frexp(level, &e);            // level = f 2^e, f in [0.5, 1), e <= 0
    const uint64_t m = (uint64_t)ldexp(f, 53);    // exact: f has 53 significant bits
    const int sh = 53 - e;
    const unsigned __int128 prod = (unsigned __int128)m * Q;
    if (sh >= 128) return prod ? 1u : 0u;
    const unsigned __int128 low = prod & ((((unsigned __int128)1) << sh) - 1);
    return (uint64_t)(prod >> sh) + (low ? 1u : 0u);
}

}  // namespace twosd
