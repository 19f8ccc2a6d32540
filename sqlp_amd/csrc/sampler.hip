// sampler.hip -- on-device scenario sampling: rand(rng, sto) of
// src/smps/smps_sto.jl:117-149, i.i.d. per element, straight into an epigraph's delta
// array in HBM (no host round trip).
//
// Element e of global scenario index g draws from Philox4x32-10 with counter
// (g_lo, g_hi, e, 0) and key (seed_lo, seed_hi) -> (x0, x1, x2, x3); u1 = u01(x0, x1),
// u2 = u01(x2, x3).  Transforms (Distributions 0.25.102 as called by the reference):
//   DISCRETE  DiscreteNonParametric(values, probs): support sorted ascending; i = 1,
//             cp = p_1; while cp <= u1 && i < n: cp += p_{++i}; value = x_i
//   NORMAL    Normal(mean, sqrt(variance)): mean + sd * z, z = sqrt(-2 log(1 - u1)) cos(2 pi u2)
//             (Box-Muller; Julia's randn is a ziggurat -- same distribution, other stream)
//   UNIFORM   Uniform(left, right): left + (right - left) * u1 (two roundings, no fma)
//   BLOCK     member e_j of a joint discrete block (dist_tables.h): every member
//             draws the words of the block's lead e_0, counter (g_lo, g_hi, e_0, 0), picks the
//             realisation i of the DISCRETE walk over the block's probabilities at u1 (by binary
//             search in the running sums) and stores V[i][j]
// The stream is a function of (seed, global index, element) only, so any sharding of the
// scenarios over ranks reproduces the same scenarios.
//
// Every kernel has two instantiations: kBlocks = false is the code of a context without blocks
// (no block table is touched, the element word is e), kBlocks = true reads the element's lead and
// handles kind 3.  launch_sample / launch_sample_plan choose by SampleParams::blocks.
#include <hip/hip_runtime.h>
#include <math.h>
#include "twosd_internal.h"
#include "philox.h"

namespace twosd {

// member e of a block at the uniform u: column ecol[e] of the realisation dist_pick finds
__device__ __forceinline__ double block_value_at(const SampleParams &S, int e, double u) {
    const DistBlock B = S.binfo[S.eblk[e]];
    const int i = dist_pick(S.bcum + B.poff, B.R, u);
    return S.bval[B.voff + i * B.n + S.ecol[e]];   // < 2^31: the table build refuses more entries
}

template <bool kBlocks>
__global__ void __launch_bounds__(256) sample_kernel(SampleParams S) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)S.N * S.k;
    if (idx >= total) return;
    const int s = (int)(idx / S.k), e = (int)(idx - (long long)s * S.k);
    const unsigned long long g = S.first_index + (unsigned long long)s;
    const int kind = S.kind[e];
    const uint32_t ew = kBlocks ? (uint32_t)S.elead[e] : (uint32_t)e;   // the element word: a block's lead
    const Philox4 r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), ew, 0u, (uint32_t)S.seed,
                                    (uint32_t)(S.seed >> 32));
    const double u1 = u01(r.v[0], r.v[1]);
    double v;
    if (kBlocks && kind == kDistBlock) {
        v = block_value_at(S, e, u1);
    } else if (kind == 0) {   // DISCRETE
        const int o = S.off[e], n = S.off[e + 1] - o;
        int i = 0;
        double cp = S.prob[o];
        while (cp <= u1 && i < n - 1) cp = __dadd_rn(cp, S.prob[o + (++i)]);
        v = S.val[o + i];
    } else if (kind == 1) {   // NORMAL
        const double u2 = u01(r.v[2], r.v[3]);
        const double z = sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2);
        v = __dadd_rn(S.p0[e], __dmul_rn(S.p1[e], z));
    } else {   // UNIFORM
        v = __dadd_rn(S.p0[e], __dmul_rn(__dadd_rn(S.p1[e], -S.p0[e]), u1));
    }
    S.out[idx] = __dadd_rn(v, -S.tmpl[e]);   // stored as the delta (value - template value)
}

hipError_t launch_sample(const SampleParams &S, hipStream_t st) {
    const long long total = (long long)S.N * S.k;
    if (total <= 0) return hipSuccess;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (S.blocks) hipLaunchKernelGGL(sample_kernel<true>, grid, dim3(256), 0, st, S);
    else hipLaunchKernelGGL(sample_kernel<false>, grid, dim3(256), 0, st, S);
    return hipGetLastError();
}

// ---- variance-reduced streams (twosd_sampling) -------------------------------
// Both keep sample_kernel's words: u1, u2 of (index, element) come from the same Philox call, so
// the streams differ from the i.i.d. one only in where each element's distribution is inverted.

// DISCRETE (kind 0) or UNIFORM (kind 2) element e at the uniform u in [0, 1]: sample_kernel's
// arithmetic.  u = 1.0 is legal: the DISCRETE walk stops at the last support point, UNIFORM gives
// `right` (up to its two roundings).
__device__ __forceinline__ double invert_at(const SampleParams &S, int e, int kind, double u) {
    if (kind == 0) {
        const int o = S.off[e], n = S.off[e + 1] - o;
        int i = 0;
        double cp = S.prob[o];
        while (cp <= u && i < n - 1) cp = __dadd_rn(cp, S.prob[o + (++i)]);
        return S.val[o + i];
    }
    return __dadd_rn(S.p0[e], __dmul_rn(__dadd_rn(S.p1[e], -S.p0[e]), u));
}

// ANTITHETIC: one thread per (scenario, element) like sample_kernel.  Pair p = g >> 1 draws the
// words of index 2p; the even member is the i.i.d. draw of 2p, the odd member inverts DISCRETE /
// UNIFORM at 1 - u1 (exact in fp64: u1 is a multiple of 2^-53 below 1) and negates NORMAL's z.
// A block's members all read the lead's words, so the odd scenario walks the block at 1 - u1.
template <bool kBlocks>
__global__ void __launch_bounds__(256) sample_antithetic_kernel(SampleParams S) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)S.N * S.k;
    if (idx >= total) return;
    const int s = (int)(idx / S.k), e = (int)(idx - (long long)s * S.k);
    const unsigned long long g = S.first_index + (unsigned long long)s, g0 = g & ~1ull;
    const bool odd = (g & 1ull) != 0;
    const int kind = S.kind[e];
    const uint32_t ew = kBlocks ? (uint32_t)S.elead[e] : (uint32_t)e;
    const Philox4 r = philox4x32_10((uint32_t)g0, (uint32_t)(g0 >> 32), ew, 0u, (uint32_t)S.seed,
                                    (uint32_t)(S.seed >> 32));
    const double u1 = u01(r.v[0], r.v[1]);
    double v;
    if (kBlocks && kind == kDistBlock) {
        v = block_value_at(S, e, odd ? 1.0 - u1 : u1);
    } else if (kind == 1) {
        const double u2 = u01(r.v[2], r.v[3]);
        const double z = sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2);
        v = __dadd_rn(S.p0[e], __dmul_rn(S.p1[e], odd ? -z : z));
    } else {
        v = invert_at(S, e, kind, odd ? 1.0 - u1 : u1);
    }
    S.out[idx] = __dadd_rn(v, -S.tmpl[e]);
}

// LHS: one thread per (block of G scenarios, element), e fastest across the lanes, so at step j a
// wave stores runs of consecutive doubles of the rows b G + j.  The thread first builds the
// (block, element) permutation of 0..G-1 by the inside-out Fisher-Yates shuffle from Philox
// counters (b_lo, b_hi, e, 2 + (i >> 2)) -- the fourth word keeps them apart from the scenario
// words (0) and the bootstrap's (1) -- then walks the block: member j inverts at
// u = min((perm[j] + u1(g, e)) / G, 1 - 2^-53), NORMAL through the inverse normal CDF (Box-Muller
// cannot be stratified in one uniform).  G + ceil(G / 4) Philox calls for G outputs.
// The permutation is bytes in LDS, [ceil(G / 4)][threads][4]: thread t owns dword column t of
// every row, so whatever entries the lanes of a wave touch in one access (the shuffle's perm[t]
// is a different row in every lane) lie in 32 distinct banks per half wave -- no conflicts, and no
// two threads ever share a dword.  128 threads x 256 bytes = 32 KB at G = 256.
// A block's permutation and u1 are those of (LHS block, lead): each of its n members rebuilds the
// same permutation and draws the same words in its own thread (n times the Philox work of one
// element; the kernel's times are in DESIGN.md §5.10, the recomputation's share of them is not
// measured), which keeps the one-thread-per-(block, element) store pattern.
constexpr int kLhsThreads = 128;
template <bool kBlocks>
__global__ void __launch_bounds__(kLhsThreads) sample_lhs_kernel(SampleParams S, int G, long long nblk) {
    extern __shared__ unsigned char lhs_perm[];
    const long long idx = (long long)blockIdx.x * kLhsThreads + threadIdx.x;
    if (idx >= nblk * S.k) return;   // no barrier below: every thread works on its own column
    const long long bl = idx / S.k;
    const int e = (int)(idx - bl * S.k);
    const unsigned long long gb = S.first_index / (unsigned long long)G + (unsigned long long)bl;
    const uint32_t k0 = (uint32_t)S.seed, k1 = (uint32_t)(S.seed >> 32);
    const uint32_t ew = kBlocks ? (uint32_t)S.elead[e] : (uint32_t)e;
    unsigned char *col = lhs_perm + 4 * threadIdx.x;
    const auto at = [&](int i) -> unsigned char & { return col[(size_t)(i >> 2) * (4 * kLhsThreads) + (i & 3)]; };
    at(0) = 0;
    Philox4 w{};
    for (int i = 1; i < G; ++i) {
        if (i == 1 || (i & 3) == 0)
            w = philox4x32_10((uint32_t)gb, (uint32_t)(gb >> 32), ew, 2u + (uint32_t)(i >> 2), k0, k1);
        const int t = (int)__umulhi(w.v[i & 3], (uint32_t)(i + 1));   // uniform on 0..i
        at(i) = at(t);
        at(t) = (unsigned char)i;
    }
    const int kind = S.kind[e];
    const double tm = S.tmpl[e], fG = (double)G;
    for (int j = 0; j < G; ++j) {
        const unsigned long long g = gb * (unsigned long long)G + (unsigned long long)j;
        const Philox4 r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), ew, 0u, k0, k1);
        const double u1 = u01(r.v[0], r.v[1]);
        double u = __ddiv_rn(__dadd_rn((double)at(j), u1), fG);
        u = u < 0x1.fffffffffffffp-1 ? u : 0x1.fffffffffffffp-1;
        double v;
        if (kBlocks && kind == kDistBlock) {
            v = block_value_at(S, e, u);
        } else if (kind == 1) {
            const double z = normcdfinv(u > 0x1p-54 ? u : 0x1p-54);
            v = __dadd_rn(S.p0[e], __dmul_rn(S.p1[e], z));
        } else {
            v = invert_at(S, e, kind, u);
        }
        S.out[(bl * G + j) * S.k + e] = __dadd_rn(v, -tm);
    }
}

hipError_t launch_sample_plan(const SampleParams &S, int mode, int G, hipStream_t st) {
    if (mode == TWOSD_SAMPLING_IID) return launch_sample(S, st);
    const long long total = (long long)S.N * S.k;
    if (total <= 0) return hipSuccess;
    if (mode == TWOSD_SAMPLING_ANTITHETIC) {
        const dim3 grid((unsigned)((total + 255) / 256));
        if (S.blocks) hipLaunchKernelGGL(sample_antithetic_kernel<true>, grid, dim3(256), 0, st, S);
        else hipLaunchKernelGGL(sample_antithetic_kernel<false>, grid, dim3(256), 0, st, S);
    } else {
        const long long nblk = S.N / G, work = nblk * S.k;
        const size_t lds = (size_t)((G + 3) / 4) * 4 * kLhsThreads;
        const dim3 grid((unsigned)((work + kLhsThreads - 1) / kLhsThreads));
        if (S.blocks) hipLaunchKernelGGL(sample_lhs_kernel<true>, grid, dim3(kLhsThreads), lds, st, S, G, nblk);
        else hipLaunchKernelGGL(sample_lhs_kernel<false>, grid, dim3(kLhsThreads), lds, st, S, G, nblk);
    }
    return hipGetLastError();
}

}  // namespace twosd
