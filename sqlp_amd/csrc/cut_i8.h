// cut_i8.h -- the fixed-point (int8-limb) operands of the cut's integer MFMA pass: the ONE
// definition of the quantisation, shared by the device kernels (cut_prep.hip, cut_argmax.hip), the host-side
// check program (tests/native/cut_i8_check.cpp) and, by restatement, the numpy model
// (tests/cut_i8_model.py).
//
// A value a with |a| <= 2^E (E its scale exponent) becomes the integer
//     q = rint(a * 2^(kQ - E)),   kQ = 7 kL - 1,   so |q| <= 2^kQ and |q - a 2^(kQ - E)| <= 1/2,
// and q is written in kL balanced radix-128 digits ("limbs", most significant first):
//     q = sum_l limb[l] * 128^(kL - 1 - l),   every |limb[l]| <= 64.
//
// Proof that no limb leaves [-64, 64] (so every limb is an int8 and a 128-term sum of limb
// products stays below 2^19).  Let q_0 = q and, for j = 0 .. kL - 2,
//     d_j = ((q_j + 64) & 127) - 64  in [-64, 63],   q_{j+1} = (q_j - d_j) / 128  (exact).
// limb[kL - 1 - j] = d_j and limb[0] = q_{kL-1}.  |q_{j+1}| <= (|q_j| + 64) / 128; with
// |q_0| <= 2^(7 kL - 1) this gives |q_1| <= 2^(7 kL - 8) + 1/2, an integer, so |q_1| <= 2^(7(kL-1) - 1),
// and by induction |q_j| <= 2^(7 (kL - j) - 1): the top limb q_{kL-1} has |.| <= 2^6 = 64.
// The extremes: |a| = 2^E gives |q| = 2^kQ exactly (top limb +-64, the others 0); a = +-0 gives
// q = 0; a denormal (or any |a| < 2^(E - kQ - 1)) gives q = 0, since the scaled value is below 1/2
// whether or not the scaling itself rounded.
//
// The scale exponents are clamped to [kEmin, ...]: a scale larger than needed stays valid
// (|a| <= 2^E still holds), it only costs resolution, and the band is computed from the clamped
// exponent.  The clamp keeps 2^(kQ - E) and the pass's fp32 output scale 2^(S + kOutShift) normal numbers.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TWOSD_I8_HD __host__ __device__ inline
#else
#define TWOSD_I8_HD inline
#endif

namespace twosd {
namespace ci8 {

#ifndef TWOSD_CUT_I8_L
#define TWOSD_CUT_I8_L 3
#endif
constexpr int kL = TWOSD_CUT_I8_L;          // limbs per operand
constexpr int kQ = 7 * kL - 1;              // |q| <= 2^kQ
constexpr int kEmin = -64;                  // lowest scale exponent used
constexpr int kPairs = kL * (kL + 1) / 2;   // kept limb pairs (l1 + l2 <= kL - 1)
// combine() weighs level lv by 128^(kL-1-lv), the product qa qd weighs it by 128^(2kL-2-lv): the
// output scale of a vertex with scale exponent S is 2^(S + kOutShift)
constexpr int kOutShift = 7 * (kL - 1) - 2 * kQ;
static_assert(kL >= 2 && kL <= 4, "2 to 4 limbs (q must fit an int32)");

// the magnitude the dropped limb pairs (l1 + l2 >= kL: both limbs are lower limbs, |.| <= 64) can
// add to one element's product qa * qd
constexpr double dropped_pairs() {
    double s = 0.0;
    for (int l1 = 1; l1 < kL; ++l1)
        for (int l2 = 1; l2 < kL; ++l2)
            if (l1 + l2 >= kL) {
                double w = 1.0;
                for (int i = 0; i < 2 * kL - 2 - l1 - l2; ++i) w *= 128.0;
                s += 64.0 * 64.0 * w;
            }
    return s;
}
constexpr double kDropped = dropped_pairs();

// the least exponent E >= kEmin with a <= 2^E (a >= 0, finite; 0 gives kEmin)
TWOSD_I8_HD int scale_exp(double a) {
    if (!(a > 0.0)) return kEmin;
    if (!(a <= 1.7976931348623157e308)) return 1024;   // infinite: the pass is not used (any value is safe)
    int e;
    const double f = frexp(a, &e);          // a = f 2^e, f in [1/2, 1)
    if (f == 0.5) --e;                      // a = 2^(e-1) exactly
    return e < kEmin ? kEmin : e;
}

// q of a at scale exponent E (|a| <= 2^E)
TWOSD_I8_HD int quantise(double a, int E) { return (int)rint(ldexp(a, kQ - E)); }

// the same q from the factor f = 2^(kQ - E) (a normal number: E >= kEmin and E <= kQ + 1022):
// a * f is the exact scaling ldexp performs, or (below the normal range) a value under 1/2
TWOSD_I8_HD int quantise_by(double a, double f) { return (int)rint(a * f); }

// the limbs of q, most significant first
TWOSD_I8_HD void limbs(int q, int8_t *out) {
    for (int j = 0; j < kL - 1; ++j) {
        const int d = ((q + 64) & 127) - 64;
        out[kL - 1 - j] = (int8_t)d;
        q = (q - d) >> 7;                   // q - d is a multiple of 128
    }
    out[0] = (int8_t)q;
}

// The pass's value of one dot product from its level sums acc[lv] = sum over the kept pairs with
// l1 + l2 = lv of sum_e limb_a[l1] limb_d[l2] (exact int32; |acc| <= kL 128 64^2 < 2^24 converts to fp32 exactly): a fixed sequence of
// fp32 operations, f = fma(f, 128, acc[lv]) from f = acc[0], then f * scale (scale = 2^(S + kOutShift)).
// Two roundings for kL = 3 (the first fma is exact below 2^24 only for small sums: counted).
TWOSD_I8_HD float combine(const int *acc, float scale) {
    float f = (float)acc[0];
    for (int lv = 1; lv < kL; ++lv) f = fmaf(f, 128.0f, (float)acc[lv]);
    return f * scale;
}

// The band term of one vertex: a bound on |combine(...) - sum_e pc_e d_e| over every scenario with
// |d_e| <= dmax_e, where pc_e = fl(PK[v,e] coef_e), E_e = scale_exp(dmax_e), u_e = pc_e 2^E_e,
// S = scale_exp(max_e |u_e|), and
//     nsum = sum_{e < k} (dmax_e 2^-E_e + |u_e| 2^-S)      (each term <= 1).
// In units of 2^(S - 2 kQ) the error is at most
//     2^(kQ-1) nsum + k/4          operand quantisation (|eps| <= 1/2 on either side)
//   + k kDropped                   the dropped limb pairs
//   + (kL - 1) 2^-24 R (1 + 2^-24) the level combination's roundings, R = k 64^2 sum_lv (lv + 1) 128^(2kL-2-lv)
//                                  >= every intermediate's magnitude
// DESIGN 5.4 has the derivation.
TWOSD_I8_HD double band_term(int k, int S, double nsum) {
    double R = 0.0, w = 1.0;
    for (int lv = kL - 1; lv >= 0; --lv) { R += (lv + 1) * w; w *= 128.0; }   // pairs per level x weight
    R *= (double)k * 64.0 * 64.0 * (double)(1 << (7 * (kL - 1)));           // in units of the product qa qd
    const double u32 = ldexp(1.0, -24);
    const double units = ldexp(nsum, kQ - 1) + 0.25 * k + (double)k * kDropped + (kL - 1) * u32 * R * (1.0 + u32);
    return ldexp(units, S - 2 * kQ);
}

}  // namespace ci8
}  // namespace twosd
