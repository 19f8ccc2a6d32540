// cut_argmax.hip -- the cut's MFMA argmax passes (the maths: cut_kernel.hip): the fp64, fp32 and
// integer pass, the tile end they share, the histogram reduce, and the integer pass's debug scores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <utility>
#include "cut_common.h"

namespace twosd {

typedef double d4 __attribute__((ext_vector_type(4)));

// Running state of one scenario row over the vertices one lane sees, in increasing vertex
// order: M = max so far, thr = band_floor(M), I = the first vertex scoring M, n = entries in
// this lane's candidate log (kCandC + 1: overflowed), f = its first entry.  The first entry
// stays in a register and is stored (log[0]) only for a row the fixup will read: most rows
// just raise their maximum past the band again and again, and each raise restarts the log.
struct RowEx { double M, thr; int I, n, f; float thr32; };

// the fp32 prefilter's floor of a row (cut_argmax3_kernel): a float at or below fl32(y) for every
// y >= pred64(thr).  A score s = fl64(base + t) >= thr has base + t >= pred64(thr); with b32 >= base
// (rounded up) and fp32 addition monotone, fl32(b32 + t) >= fl32(pred64(thr)) >= this floor.
// f = RN32(thr) is within one float step of RD32(pred64(thr)); f - |f| 2^-21 (rounded) lies at least
// three float steps lower, and the 2^-140 covers the subnormal range.  -inf stays -inf; past FLT_MAX
// the floor is FLT_MAX (every y there rounds to +inf)
__device__ __forceinline__ float thr32_of(double thr) {
    const float f = (float)thr;
    if (f == INFINITY) return 3.40282347e38f;
    return fmaf(-fabsf(f), 0x1p-21f, f) - 0x1p-140f;
}

// s >= thr: s enters the band of the running max (or raises it).  HOLD: the first entry is kept
// in b.f (stored at the end of the tile for the rows the fixup reads); otherwise it is stored at
// once (the instantiations at 3 blocks per CU have no register to spare for it)
template <bool HOLD>
__device__ __forceinline__ void row_log(RowEx &b, double s, int v, double rel, double band, int *lbase, unsigned lo) {
    if (s == -INFINITY) return;                  // padding vertices (-inf base row) never enter
    // the 3-blocks build: an opaque copy, so the entry addresses are formed here, on this rare path,
    // instead of being hoisted out of the chunk loop as 64-bit values that would spill
    if (!HOLD) asm volatile("" : "+v"(lo));
    const double tn = band_floor(s, rel, band);
    if (tn > b.M) {                              // every earlier entry is below the band for good
        if (HOLD) b.f = v;
        else lbase[lo] = v;
        b.n = 1;
    } else {
        if (HOLD && b.n == 0) b.f = v;
        else if (b.n < kCandC) lbase[lo + b.n] = v;
        b.n = min(b.n + 1, kCandC + 1);
    }
    if (s > b.M) { b.M = s; b.I = v; b.thr = tn; b.thr32 = thr32_of(tn); }
}

template <bool HOLD>
__device__ __forceinline__ void row_fast(RowEx &b, double s, int v, double rel, double band, int *lbase, unsigned lo) {
    if (__builtin_expect(s >= b.thr, 0)) row_log<HOLD>(b, s, v, rel, band, lbase, lo);
}

// ---- v2: the score tile transposed -- MFMA A operand = the staged vertex chunk, B operand =
// the scenario deltas -- so the C/D layout puts one SCENARIO per lane column (j) and four
// vertices per lane (rows g + 4r): a lane tracks the running argmax of ONE scenario per A tile
// instead of four, which frees the registers for two scenario tiles per wave (32 scenarios,
// 128 per block) and two vertex tiles per chunk (32 vertices): every chunk staged in LDS
// serves twice the scenarios of v1, and each LDS fragment read feeds two MFMAs.  The deltas
// stay raw in registers (coef_e(x) is folded into the staged chunk), so the S_e sums of the
// cut reuse them instead of re-reading the deltas from HBM.  Chunks are double-buffered.
#ifndef TWOSD_CUT_KG
#define TWOSD_CUT_KG 6                   // k-blocks whose fragments are read ahead together
#endif
#ifndef TWOSD_CUT_SB
#define TWOSD_CUT_SB 1                   // scheduling barrier between the groups
#endif
constexpr int kLdsRow2 = 32;             // doubles per k-row of a chunk

// LDS position of (k-row kk, vertex vv): odd rows have their 16-double halves swapped, so the
// two k-rows a half-wave reads together (g = 0, 1 / 2, 3) fall on disjoint banks
__device__ __forceinline__ int lds2(int kk, int vv) { return kk * kLdsRow2 + (vv ^ ((kk & 1) << 4)); }

// The value of a decided row in fp64, the same bits in every pass, split and kernel: base[I] + t,
// t = (c_0 + c_1) + (c_2 + c_3), c_g the fma chain over e = g, g + 4, g + 8, ... < k of
// (PK[I,e] coef_e) dv_e from 0.  cut_tile_end's pick_terms forms lane (g, .)'s c_g from its deltas of
// k-block kb (e = 4 kb + g); dec_combine the xor-16 / xor-32 sum that forms t on every lane of the column.
__device__ __forceinline__ double dec_combine(double c) {
    c += __shfl_xor(c, 16);
    return c + __shfl_xor(c, 32);
}

// Combine the 4 lanes (g) of a scenario column: the row maximum M, and for each lane the number
// of its logged entries that can lie in the band of M (0 when the lane's own max is below the
// band floor).  tot == 1: the row is decided, its pick the first vertex of the one lane that
// reaches the band; otherwise the row is re-decided from the logs, whose lengths `pack` holds
// (kCandBits per lane group; kCandC + 1 = overflowed).  Every lane of the column ends with the result.
__device__ __forceinline__ void combine_ex(RowEx &rb, double rel, double band, int g, int &pack, int &tot) {
    double M = rb.M;
    M = fmax(M, __shfl_xor(M, 16));
    M = fmax(M, __shfl_xor(M, 32));
    const double thr = band_floor(M, rel, band);
    const int n = (rb.M != -INFINITY && rb.M >= thr) ? rb.n : 0;
    int pk = n << (kCandBits * g);
    tot = n;
    int it = n ? rb.I : 0x7fffffff;
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        tot += __shfl_xor(tot, o);
        pk |= __shfl_xor(pk, o);
        it = min(it, __shfl_xor(it, o));
    }
    rb.M = M;
    rb.I = (M == -INFINITY || it == 0x7fffffff) ? -1 : it;
    pack = pk;
}

// ---- The steps the MFMA passes (cut_argmax2 / 3 / 4_kernel) share.  A pass keeps its operand load
// and quantisation, its LDS, `stage`, the chunk product and where the candidate steps run relative
// to the MFMAs.  These kernels sit on their register caps, and the compiler's allocation follows how
// the source is cut: what is a function below is what left every instantiation's occupancy, LDS and
// chunk-loop scratch traffic as they were (profiles/r11).

// One work unit of the persistent grid as a wave sees it, for cut_tile_end: a whole scenario tile or
// vertex range `range` of a tail tile; the wave's scenarios are s0 + j (row 0) and s0 + 16 + j
// (row 1); lane (g, j)'s candidate logs of the two are lbase[log0 ...] and lbase[log0 + lstep ...].
struct CutUnit {
    bool tail;
    int range, s0;
    int *lbase;
    unsigned log0, lstep;
};

__device__ __forceinline__ int cut_num_units(const CutParams &P) {
    const int ntiles = (P.N + kCutTile2 - 1) / kCutTile2;
    return P.full_units + (ntiles - P.full_units) * P.tail_S;
}

__device__ __forceinline__ RowEx row_ex_init() {
    RowEx b;
    b.M = -INFINITY; b.thr = -INFINITY; b.I = -1; b.n = 0; b.f = 0; b.thr32 = -INFINITY;
    return b;
}

// The fp64 delta of k-block kb (element e = 4 kb + g < k) of a finished tile's scenario, from one of
// two sources: the fp64 pass's delta registers, or (an int: the scenario) the deltas read again.
template <int KB>
__device__ __forceinline__ double tile_delta(const CutParams &, const double (&a)[KB], int kb, int) { return a[kb < KB ? kb : KB - 1]; }
template <int KB>
__device__ __forceinline__ double tile_delta(const CutParams &P, int sx, int, int e) { return sx < P.N ? P.dv[(size_t)sx * P.k + e] : 0.0; }

// The end of a unit: the 4 lanes of each row combined; the held first log entries stored for the
// rows the fixup reads (every tail row: the merge decides); the picks translated to vertex indices
// (the logs keep vmap positions: the fixup translates them).  A tail range leaves its result in
// tp_* for cut_tail_merge_kernel: the log lengths of the range's band, since the merge decides with
// the band of the row's maximum over all ranges (a range below it contributes nothing).  A whole
// tile writes arg / val / flag -- a decided row's value is the pick's fp64 value (pick_terms), a
// flagged row keeps the pass's maximum and the fixup writes its restated value -- and adds p * val
// and the vertex histogram with its scenarios in order (lane 0 reads them from lanes 0-15).
// d0 / d1: the two rows' delta sources (tile_delta); the arithmetic and its order are the same for both.
template <int KB, bool HOLD, typename Src>
__device__ __forceinline__ void cut_tile_end(const CutParams &P, const CutUnit &u, RowEx &rb0, RowEx &rb1, const Src &d0, const Src &d1,
                                             double rel, double band, int lane, double &pv_sum, double (&Sacc)[2]) {
    extern __shared__ unsigned long long hl[];   // the block's LDS histogram (P.hist_lds)
    const int g = lane >> 4, j = lane & 15;
    int pk0, pk1, nt0, nt1;
    combine_ex(rb0, rel, band, g, pk0, nt0);
    combine_ex(rb1, rel, band, g, pk1, nt1);
    if (HOLD && rb0.n > 0 && (u.tail || nt0 >= 2)) u.lbase[u.log0] = rb0.f;
    if (HOLD && rb1.n > 0 && (u.tail || nt1 >= 2)) u.lbase[u.log0 + u.lstep] = rb1.f;
    rb0.I = rb0.I >= 0 ? P.vmap[rb0.I] : -1;
    rb1.I = rb1.I >= 0 ? P.vmap[rb1.I] : -1;
    const int sa = u.s0 + j, sb = u.s0 + 16 + j;
    if (u.tail) {
        if (g == 0) {
            const int t0 = P.full_units * kCutTile2;
            if (sa < P.N) {
                const size_t o = (size_t)(sa - t0) * P.tail_S + u.range;
                P.tp_m[o] = rb0.M; P.tp_i[o] = rb0.I; P.tp_f[o] = pk0;
            }
            if (sb < P.N) {
                const size_t o = (size_t)(sb - t0) * P.tail_S + u.range;
                P.tp_m[o] = rb1.M; P.tp_i[o] = rb1.I; P.tp_f[o] = pk1;
            }
        }
        return;
    }
    if (nt0 < 2) pk0 = 0;   // decided
    if (nt1 < 2) pk1 = 0;
    const bool ok0 = sa < P.N && !pk0 && rb0.I >= 0, ok1 = sb < P.N && !pk1 && rb1.I >= 0;
    const double p0 = ok0 ? P.w[sa] * P.inv_total : 0.0, p1 = ok1 ? P.w[sb] * P.inv_total : 0.0;
    // one scenario and its pick ai (weight pp; ok: decided): the S_e terms p_w PK[a(w), e] dv[w, e] --
    // lane (g, j) holds scenario j's e = 4 kb + g, the 16 scenarios of a tile are summed by a fixed xor
    // tree, lane (g, kb mod 16) keeps the sum in Sacc -- and the lane's chain c_g of the decided value
    // (dec_combine); returns t.  The k-blocks go in groups of 6, their loads in flight together
    auto pick_terms = [&](const Src &d, bool ok, int ai, double pp) -> double {
        const double *pk = P.PK + (size_t)(ai >= 0 ? ai : 0) * P.k4;
        const double pu = ok ? pp : 0.0;
        constexpr int FG = 6;
        double cg = 0.0;
#pragma unroll
        for (int k0 = 0; k0 < KB; k0 += FG) {
            double d64[FG], pke[FG];
#pragma unroll
            for (int q = 0; q < FG; ++q) {
                const int e = 4 * (k0 + q) + g;
                const bool in = k0 + q < KB && e < P.k;
                d64[q] = in ? tile_delta<KB>(P, d, k0 + q, e) : 0.0;
                pke[q] = in ? pk[e] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < FG; ++q) {
                const int kb = k0 + q, e = 4 * kb + g;
                if (kb >= KB) break;
                if (e < P.k) cg = fma(pke[q] * P.coef[e], d64[q], cg);
                double v = (e < P.k) ? pu * pke[q] * d64[q] : 0.0;
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
                if (j == (kb & 15)) {
                    if (kb < 16) Sacc[0] += v;
                    else Sacc[1] += v;
                }
            }
        }
        return dec_combine(cg);
    };
    const double tv0 = pick_terms(d0, ok0, rb0.I, p0);
    const double tv1 = pick_terms(d1, ok1, rb1.I, p1);
    const double vl0 = ok0 ? P.base[rb0.I] + tv0 : rb0.M, vl1 = ok1 ? P.base[rb1.I] + tv1 : rb1.M;
    if (g == 0) {
        if (sa < P.N) { P.arg[sa] = rb0.I; P.val[sa] = vl0; P.flag[sa] = pk0; }
        if (sb < P.N) { P.arg[sb] = rb1.I; P.val[sb] = vl1; P.flag[sb] = pk1; }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
            const int ok = __shfl(t == 0 ? (int)ok0 : (int)ok1, jj);
            const int ai = __shfl(t == 0 ? rb0.I : rb1.I, jj);
            const double pp = __shfl(t == 0 ? p0 : p1, jj);
            const double vl = __shfl(t == 0 ? vl0 : vl1, jj);
            if (lane == 0 && ok) {
                pv_sum = fma(pp, vl, pv_sum);
                const unsigned long long hq = (unsigned long long)__double2ull_rn(pp * kFix);
                if (P.hist_lds) __hip_atomic_fetch_add(&hl[ai], hq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else atomicAdd(&P.hist[ai], hq);
            }
        }
    }
}

#ifndef TWOSD_CUT_LB3
#define TWOSD_CUT_LB3 1                  // 3 blocks per CU for KB <= 22 (168 VGPRs; ssn: 62 -> 76 % of the roofline)
#endif
template <int KB>
__global__ void __launch_bounds__(256, (TWOSD_CUT_LB3 && KB <= 22) ? 3 : 2) cut_argmax2_kernel(CutParams P) {
    if (*P.mode != 0) return;                       // the fp32 pass runs this cut (cut_argmax3_kernel)
    __shared__ double Bs[2][4 * KB * kLdsRow2];     // double-buffered chunk (k-major)
    constexpr bool kHold = !(TWOSD_CUT_LB3 && KB <= 22);   // a register for the logs' first entries (2 blocks per CU)
    extern __shared__ unsigned long long hl[];      // nv entries when P.hist_lds
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: scalar staging loop
    if (P.hist_lds)
        for (int v = threadIdx.x; v < P.nv; v += 256) hl[v] = 0ull;
    const int g = lane >> 4, j = lane & 15;
    const int nchunks = (*P.nvc + kVT2 - 1) / kVT2;   // the argmax's vertices (vmap)
    const int nunits = cut_num_units(P);
    const double band = kHold ? __longlong_as_double((long long)*P.band_bits) : cut_band_scalar(P);
    const double rel = P.tie_rel;
    double pv_sum = 0.0;
    double Sacc[2] = {0.0, 0.0};   // lane (g, j): e = 4 kb + g for kb = j, j + 16

    for (int unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        // a whole tile (all vertex chunks), or vertex range `range` of a tail tile.  (This unit arithmetic
        // stays written in each pass: as one function next to cut_tile_end it took the fp32 pass from
        // 0 / 1 / 2 scratch loads per chunk step to 1 / 2 / 3 at KB 12-16 / 22-24 / 32.)
        const bool tail = unit >= P.full_units;
        const int tile = tail ? P.full_units + (unit - P.full_units) / P.tail_S : unit;
        const int range = tail ? (unit - P.full_units) % P.tail_S : 0;
        const int c_lo = tail ? (int)((long long)nchunks * range / P.tail_S) : 0;
        const int c_hi = tail ? (int)((long long)nchunks * (range + 1) / P.tail_S) : nchunks;
        // this wave: scenarios s0 + j (tile 0) and s0 + 16 + j (tile 1); lane (g, j) holds their
        // deltas e = 4 kb + g (the B operand: k = g, column = j)
        const int s0 = tile * kCutTile2 + wid * 32;
        double a0[KB], a1[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            const int e = 4 * kb + g;
            const int sa = s0 + j, sb = s0 + 16 + j;
            a0[kb] = (sa < P.N && e < P.k) ? P.dv[(size_t)sa * P.k + e] : 0.0;
            a1[kb] = (sb < P.N && e < P.k) ? P.dv[(size_t)sb * P.k + e] : 0.0;
            if (e == P.k) a0[kb] = a1[kb] = 1.0;   // x the base row of the chunk
        }
        RowEx rb0 = row_ex_init(), rb1 = rb0;   // scenario s0 + j / s0 + 16 + j over this lane's vertices v0 + g + 4r (+16)
        // this lane's candidate logs of the two scenarios (rows padded to whole tiles)
        // (a wave-uniform base and a 32-bit element offset: one VGPR per lane instead of a pointer pair)
        int *const lbase = tail ? P.tcand : P.cand;
        const unsigned log0 = tail ? (unsigned)(((((size_t)(s0 + j - P.full_units * kCutTile2)) * P.tail_S + range) * 4 + g) * kCandC)
                                      : (unsigned)((((size_t)(s0 + j)) * 4 + g) * kCandC);
        const unsigned lstep = 16u * (tail ? P.tail_S : 1) * 4 * kCandC;   // scenario + 16

        // chunk staging by LDS-DMA (global_load_lds_dwordx4, no VGPR round trip): instruction i
        // of the chunk writes k-rows 4i .. 4i+3 (1 KiB, lane-linear), lane L the 16 bytes of
        // row 4i + L/16 at LDS position 2 (L % 16); the source vertex pair is that position with
        // the row's half swap (lds2) applied, so the image is exactly lds2's layout
        auto stage = [&](int buf, int v0) {
            for (int i = wid; i < KB; i += 4) {
                const int kk = 4 * i + (lane >> 4);
                const int vv = (2 * (lane & 15)) ^ ((kk & 1) << 4);
                __builtin_amdgcn_global_load_lds((const void *)(P.PKTc + (size_t)kk * P.vcap32 + v0 + vv),
                                                 (__attribute__((address_space(3))) void *)&Bs[buf][i * 4 * kLdsRow2], 16, 0, 0);
            }
        };
        stage(0, c_lo * kVT2);
        __syncthreads();            // chunk c_lo landed (the barrier drains the DMA)
        for (int ch = c_lo; ch < c_hi; ++ch) {
            const int buf = (ch - c_lo) & 1;
            const int v0 = ch * kVT2;
            // chunk ch+1 into the other buffer while this one is multiplied (its readers passed
            // the last barrier)
            if (ch + 1 < c_hi) stage(buf ^ 1, v0 + kVT2);
            d4 c00 = {0.0, 0.0, 0.0, 0.0}, c01 = c00, c10 = c00, c11 = c00;   // c[vertex tile][scenario tile]
            // fragments are read in groups of KG k-blocks ahead of their MFMAs; the scheduling
            // barrier keeps the compiler from hoisting every read of the chunk (register spills)
            constexpr int KG = TWOSD_CUT_KG;
#pragma unroll
            for (int k0 = 0; k0 < KB; k0 += KG) {
                double x0[KG], x1[KG];
#pragma unroll
                for (int u = 0; u < KG; ++u) {
                    if (k0 + u < KB) {
                        x0[u] = Bs[buf][lds2(4 * (k0 + u) + g, j)];
                        x1[u] = Bs[buf][lds2(4 * (k0 + u) + g, 16 + j)];
                    }
                }
#pragma unroll
                for (int u = 0; u < KG; ++u) {
                    if (k0 + u < KB) {
                        c00 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[u], a0[k0 + u], c00, 0, 0, 0);
                        c01 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[u], a1[k0 + u], c01, 0, 0, 0);
                        c10 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[u], a0[k0 + u], c10, 0, 0, 0);
                        c11 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[u], a1[k0 + u], c11, 0, 0, 0);
                    }
                }
                if (TWOSD_CUT_SB) __builtin_amdgcn_sched_barrier(0);
            }
            // C/D: register r of a tile is vertex row g + 4r, scenario column j; this lane's
            // vertices in increasing order: v0 + g + 4r, then v0 + 16 + g + 4r.  The scores
            // include the base (-inf past nv).
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                row_fast<kHold>(rb0, c00[r], v0 + g + 4 * r, rel, band, lbase, log0);
                row_fast<kHold>(rb1, c01[r], v0 + g + 4 * r, rel, band, lbase, log0 + lstep);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                row_fast<kHold>(rb0, c10[r], v0 + 16 + g + 4 * r, rel, band, lbase, log0);
                row_fast<kHold>(rb1, c11[r], v0 + 16 + g + 4 * r, rel, band, lbase, log0 + lstep);
            }
            __syncthreads();
        }
        const CutUnit un = {tail, range, s0, lbase, log0, lstep};
        cut_tile_end<KB, kHold>(P, un, rb0, rb1, a0, a1, rel, band, lane, pv_sum, Sacc);   // from the delta registers
    }
    // (the block end stays written in each pass: as one function it raised this pass's scratch from 32 to
    // 172 bytes per lane at KB 22, from 0 to 24-268 at KB 24-32, and the fp32 pass's from 72 to 628 at KB 30)
    if (P.hist_lds) {
        __syncthreads();
        for (int v = threadIdx.x; v < P.nv; v += 256) P.hist_part[(size_t)blockIdx.x * P.nv + v] = hl[v];
    }
    const int slot = blockIdx.x * 4 + wid;
    double *out = P.partial + (size_t)slot * (P.k + 1);
    if (lane == 0) out[0] = pv_sum;
    // lane (g, j) owns e = 4 j + g (kb = j) and e = 4 (j + 16) + g (kb = j + 16)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int e = 4 * (j + 16 * t) + g;
        if (e < P.k) out[1 + e] = Sacc[t];
    }
}

// ---- v3: the fp32 MFMA pass (v_mfma_f32_16x16x4f32: twice the fp64 rate on gfx950, an exact
// fmaf chain).  The layout of v2 with fp32 operands: the vertex chunk (coef_e(x) PK rows rounded
// to fp32, no base row) DMA'd into LDS, the scenario deltas rounded to fp32 in registers.  The
// MFMA gives t32 ~ sum_e PK[v,e] coef_e dv[w,e]; the score is base[v] + t32 in fp64 (the base is
// the restatement's own fp64 value), within the fp32 band of the restated score
// (cut_vbase_kernel), and the decisions, logs, tail ranges and fixup are those of v2 with that
// band.  The f32 C/D layout: register r of a tile is vertex row 4g + r, scenario column j.  At the
// end of a tile the two scenarios' fp64 deltas are read again for the S_e sums and the decided
// rows' values (fp64, from the pick's PK row).
constexpr int kLdsRow3 = 32;             // floats per k-row of an fp32 chunk (32 vertices)
// LDS position of (k-row kk, vertex vv): a 128-byte k-row puts rows kk and kk + 2 on the same
// banks, so rows with (kk >> 1) odd have their 16-float halves swapped: the four k-rows a wave
// reads together (g = 0..3) fall on disjoint banks
__device__ __forceinline__ int lds3(int kk, int vv) { return kk * kLdsRow3 + (vv ^ (((kk >> 1) & 1) << 4)); }

typedef float f4 __attribute__((ext_vector_type(4)));
#ifndef TWOSD_CUT3_BPC
#define TWOSD_CUT3_BPC 3                 // blocks per CU the fp32 pass is compiled for (2: storm cut 11.0 ms, ssn 4.7; 3: 10.6, 3.6)
#endif

template <int KB>
__global__ void __launch_bounds__(256, TWOSD_CUT3_BPC) cut_argmax3_kernel(CutParams P) {
    if (*P.mode != 1) return;                       // the fp64 pass runs this cut (cut_argmax2_kernel)
    // the logs' first entries held in a register (as cut_argmax2_kernel at 2 blocks per CU): most
    // candidate steps restart a log, and a held entry is stored only for the rows the fixup reads
#ifndef TWOSD_CUT3_HOLD
#define TWOSD_CUT3_HOLD 1                // first log entries in a register (storm argmax 8.28 -> 8.14 ms at 3 blocks per CU)
#endif
    constexpr bool kHold3 = TWOSD_CUT3_HOLD;
    constexpr int KR = kr32(KB);
    __shared__ float Bs[2][KR * kLdsRow3];          // double-buffered chunk (k-major)
    __shared__ double Bb[3][kVT2];                  // the chunks' fp64 bases (ring of 3: finish reads chunk ch - 1)
    extern __shared__ unsigned long long hl[];      // nv entries when P.hist_lds
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (P.hist_lds)
        for (int v = threadIdx.x; v < P.nv; v += 256) hl[v] = 0ull;
    const int g = lane >> 4, j = lane & 15;
    const int nvc = *P.nvc;
    const int nchunks = (nvc + kVT2 - 1) / kVT2;
    const int nunits = cut_num_units(P);
    const double band = cut_band_scalar(P);
    const double rel = P.tie_rel;
    double pv_sum = 0.0;
    double Sacc[2] = {0.0, 0.0};   // lane (g, j): e = 4 kb + g for kb = j, j + 16
#ifdef TWOSD_CUT3_COUNT
    unsigned long long cnt_steps = 0, cnt_rare = 0, cnt_lanes = 0;
#endif

    for (int unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const bool tail = unit >= P.full_units;
        const int tile = tail ? P.full_units + (unit - P.full_units) / P.tail_S : unit;
        const int range = tail ? (unit - P.full_units) % P.tail_S : 0;
        const int c_lo = tail ? (int)((long long)nchunks * range / P.tail_S) : 0;
        const int c_hi = tail ? (int)((long long)nchunks * (range + 1) / P.tail_S) : nchunks;
        const int s0 = tile * kCutTile2 + wid * 32;
        const int sa = s0 + j, sb = s0 + 16 + j;
        float a0[KB], a1[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            const int e = 4 * kb + g;
            a0[kb] = (sa < P.N && e < P.k) ? (float)P.dv[(size_t)sa * P.k + e] : 0.0f;
            a1[kb] = (sb < P.N && e < P.k) ? (float)P.dv[(size_t)sb * P.k + e] : 0.0f;
        }
        RowEx rb0 = row_ex_init(), rb1 = rb0;
        int *const lbase = tail ? P.tcand : P.cand;
        const unsigned log0 = tail ? (unsigned)(((((size_t)(s0 + j - P.full_units * kCutTile2)) * P.tail_S + range) * 4 + g) * kCandC)
                                      : (unsigned)((((size_t)(s0 + j)) * 4 + g) * kCandC);
        const unsigned lstep = 16u * (tail ? P.tail_S : 1) * 4 * kCandC;

        // LDS-DMA staging (global_load_lds_dwordx4): instruction i writes k-rows 8i .. 8i+7 (1 KiB,
        // lane-linear), lane L the 4 floats at LDS position 4 (L % 8) of row 8i + L/8; the source
        // vertices are that position with lds3's half swap applied
        auto stage = [&](int buf, int bslot, int v0) {
            for (int i = wid; i < KR / 8; i += 4) {
                const int kk = 8 * i + (lane >> 3);
                const int vv = (4 * (lane & 7)) ^ (((kk >> 1) & 1) << 4);
                __builtin_amdgcn_global_load_lds((const void *)(P.PKTc32 + (size_t)kk * P.vcap32 + v0 + vv),
                                                 (__attribute__((address_space(3))) void *)&Bs[buf][i * 8 * kLdsRow3], 16, 0, 0);
            }
            // the 32 fp64 bases (256 bytes: lanes 0..15 of the last wave, 16 bytes each)
            if (wid == 3 && lane < 16)
                __builtin_amdgcn_global_load_lds((const void *)(P.basec + v0 + 2 * lane),
                                                 (__attribute__((address_space(3))) void *)&Bb[bslot][0], 16, 0, 0);
        };
        // this lane's 8 vertices of a chunk (positions v0 + 4g + r, v0 + 16 + 4g + r) as prefilter
        // bases (basec32: rounded up, -inf past the argmax's vertices), two 16-byte loads issued one
        // chunk ahead of their use
        auto load_bases = [&](float (&bq)[8], int v0) {
            const f4 lo = *reinterpret_cast<const f4 *>(P.basec32 + v0 + 4 * g);
            const f4 hi = *reinterpret_cast<const f4 *>(P.basec32 + v0 + 16 + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) { bq[r] = lo[r]; bq[4 + r] = hi[r]; }
        };
        // the chunk's 16 scores of this lane, finished one chunk late (under chunk ch + 1's MFMAs).
        // Prefilter in fp32: b32 + t >= thr32 for every score the fp64 test (base + t >= thr, t the
        // MFMA's fp32 value) accepts (thr32_of); most chunks raise no row's band floor, so one
        // wave-wide test skips the rest.  A lane past it re-scores its 8 vertices exactly (fp64
        // bases) and runs the decisions in vertex order
        auto finish = [&](const f4 &q00, const f4 &q01, const f4 &q10, const f4 &q11, const float (&bb)[8], int vb, int bslot) {
            // per row, the bit mask of this lane's vertices (r = 0..7, increasing vertex order) past
            // the prefilter
            unsigned m0 = 0, m1 = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                m0 |= (unsigned)(bb[r] + q00[r] >= rb0.thr32) << r;
                m1 |= (unsigned)(bb[r] + q01[r] >= rb1.thr32) << r;
                m0 |= (unsigned)(bb[4 + r] + q10[r] >= rb0.thr32) << (4 + r);
                m1 |= (unsigned)(bb[4 + r] + q11[r] >= rb1.thr32) << (4 + r);
            }
#ifdef TWOSD_CUT3_COUNT
            ++cnt_steps;
            if (__builtin_amdgcn_ballot_w64((m0 | m1) != 0) != 0) { ++cnt_rare; cnt_lanes += __popcll(__builtin_amdgcn_ballot_w64((m0 | m1) != 0)); }
#endif
            // the exact steps, one passing vertex per row and lane per round (lowest first: each
            // row still sees its vertices in increasing order), the fp64 base from the chunk's LDS slot
            while (__builtin_amdgcn_ballot_w64((m0 | m1) != 0) != 0) {
                const int r0 = m0 ? __builtin_ctz(m0) : 0, r1 = m1 ? __builtin_ctz(m1) : 0;
                const int o0 = (r0 >> 2) * 16 + 4 * g + (r0 & 3), o1 = (r1 >> 2) * 16 + 4 * g + (r1 & 3);
                const double b0 = Bb[bslot][o0], b1 = Bb[bslot][o1];
                const float t0 = r0 < 4 ? q00[r0 & 3] : q10[r0 & 3];
                const float t1 = r1 < 4 ? q01[r1 & 3] : q11[r1 & 3];
                const double s0 = (vb + o0 < nvc ? b0 : -INFINITY) + (double)t0;
                const double s1 = (vb + o1 < nvc ? b1 : -INFINITY) + (double)t1;
                if (m0) row_fast<kHold3>(rb0, s0, vb + o0, rel, band, lbase, log0);
                if (m1) row_fast<kHold3>(rb1, s1, vb + o1, rel, band, lbase, log0 + lstep);
                m0 &= m0 - 1;
                m1 &= m1 - 1;
            }
        };
        f4 p00 = {0.0f, 0.0f, 0.0f, 0.0f}, p01 = p00, p10 = p00, p11 = p00;
        float bp[8];
        int pv0 = 0;
        stage(0, 0, c_lo * kVT2);
        __syncthreads();
        int bs = 0, bsp = 0;   // base ring slots of chunks ch and ch - 1
        for (int ch = c_lo; ch < c_hi; ++ch) {
            const int buf = (ch - c_lo) & 1;
            const int v0 = ch * kVT2;
            float bq[8];
            load_bases(bq, v0);                     // in flight under the MFMAs
            if (ch + 1 < c_hi) stage(buf ^ 1, bs == 2 ? 0 : bs + 1, v0 + kVT2);
            f4 c00 = {0.0f, 0.0f, 0.0f, 0.0f}, c01 = c00, c10 = c00, c11 = c00;
            constexpr int KG = TWOSD_CUT_KG;
#pragma unroll
            for (int k0 = 0; k0 < KB; k0 += KG) {
                float x0[KG], x1[KG];
#pragma unroll
                for (int u = 0; u < KG; ++u) {
                    if (k0 + u < KB) {
                        x0[u] = Bs[buf][lds3(4 * (k0 + u) + g, j)];
                        x1[u] = Bs[buf][lds3(4 * (k0 + u) + g, 16 + j)];
                    }
                }
#pragma unroll
                for (int u = 0; u < KG; ++u) {
                    if (k0 + u < KB) {
                        c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[u], a0[k0 + u], c00, 0, 0, 0);
                        c01 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0[u], a1[k0 + u], c01, 0, 0, 0);
                        c10 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[u], a0[k0 + u], c10, 0, 0, 0);
                        c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1[u], a1[k0 + u], c11, 0, 0, 0);
                    }
                }
                if (TWOSD_CUT_SB) __builtin_amdgcn_sched_barrier(0);
            }
            if (ch > c_lo) finish(p00, p01, p10, p11, bp, pv0, bsp);   // the previous chunk, under these MFMAs
            p00 = c00; p01 = c01; p10 = c10; p11 = c11;
#pragma unroll
            for (int r = 0; r < 8; ++r) bp[r] = bq[r];
            pv0 = v0;
            bsp = bs;
            bs = bs == 2 ? 0 : bs + 1;
            __syncthreads();
        }
        if (c_hi > c_lo) finish(p00, p01, p10, p11, bp, pv0, bsp);
        const CutUnit un = {tail, range, s0, lbase, log0, lstep};
        cut_tile_end<KB, kHold3>(P, un, rb0, rb1, sa, sb, rel, band, lane, pv_sum, Sacc);   // the fp64 deltas read again
    }
    if (P.hist_lds) {
        __syncthreads();
        for (int v = threadIdx.x; v < P.nv; v += 256) P.hist_part[(size_t)blockIdx.x * P.nv + v] = hl[v];
    }
#ifdef TWOSD_CUT3_COUNT
    if (lane == 0 && P.fstats) {
        atomicAdd(&P.fstats[CS_F32_STEPS], cnt_steps); atomicAdd(&P.fstats[CS_F32_RARE], cnt_rare);
        atomicAdd(&P.fstats[CS_F32_LANES], cnt_lanes);
    }
#endif
    const int slot = blockIdx.x * 4 + wid;
    double *out = P.partial + (size_t)slot * (P.k + 1);
    if (lane == 0) out[0] = pv_sum;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int e = 4 * (j + 16 * t) + g;
        if (e < P.k) out[1 + e] = Sacc[t];
    }
}

// ---- v4: the integer MFMA pass (v_mfma_i32_16x16x64_i8).  Both operands are fixed-point numbers
// of ci8::kL signed limbs (cut_i8.h): the vertex side pc_e = PK[v,e] coef_e at the scale
// 2^(S_v - E_e), the scenario deltas at 2^E_e, E_e from the epigraph's dmax cache.  The dot product
// is the sum of the limb-pair products; the pairs with l1 + l2 <= kL - 1 are kept, one exact int32
// accumulator per level l1 + l2, and ci8::combine folds the levels into the fp32 term t.  The
// score is base[v] + t in fp64 as in v3, within the integer band of the restated score
// (cut_vbase_kernel, band_bits[BAND_I8]); everything after t -- prefilter, exact steps, logs, tail
// ranges, the fp64 re-read at the tile end -- is v3's (a second copy of it: see the notes in the
// kernel).  The i32 C/D layout is the f32 one: register
// r of a tile is vertex row 4g + r, scenario column j.  An integer sum does not depend on the order
// of its terms, so the result is the same bits on any hardware and in the numpy model.

// lane (g, .)'s quantised deltas of scenario s: per k-step and limb the 16 bytes e = 64 ks + 16 g + b
// (the MFMA's B operand), from the fp64 deltas
template <int KS>
__device__ __forceinline__ void i8_quant_deltas(const CutParams &P, int s, int g, i4 (&d)[KS][ci8::kL]) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        unsigned wd[ci8::kL][4] = {};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const int e = 64 * ks + 16 * g + b;
            const double x = (s < P.N && e < P.k) ? P.dv[(size_t)s * P.k + e] : 0.0;
            int8_t lb[ci8::kL];
            ci8::limbs(ci8::quantise_by(x, P.dsc[e]), lb);
#pragma unroll
            for (int l = 0; l < ci8::kL; ++l) wd[l][b >> 2] |= (unsigned)(uint8_t)lb[l] << (8 * (b & 3));
        }
#pragma unroll
        for (int l = 0; l < ci8::kL; ++l) d[ks][l] = i4{(int)wd[l][0], (int)wd[l][1], (int)wd[l][2], (int)wd[l][3]};
    }
}

// the level sums of one chunk image (LDS or global) against one scenario tile: acc[level][vertex
// tile].  One scenario tile at a time halves the live accumulators (24 registers for kL = 3); the
// second tile reads the fragments from LDS again.
template <int KS>
__device__ __forceinline__ void i8_chunk_mma(const int8_t *img, int g, int j, const i4 (&d)[KS][ci8::kL], i4 (&acc)[ci8::kL][2]) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
        for (int l1 = 0; l1 < ci8::kL; ++l1) {
            const i4 x0 = *reinterpret_cast<const i4 *>(img + i8_frag_off(KS, l1, ks, g, j));
            const i4 x1 = *reinterpret_cast<const i4 *>(img + i8_frag_off(KS, l1, ks, g, 16 + j));
#pragma unroll
            for (int l2 = 0; l1 + l2 < ci8::kL; ++l2) {
                i4 *a = acc[l1 + l2];
                a[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(x0, d[ks][l2], a[0], 0, 0, 0);
                a[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(x1, d[ks][l2], a[1], 0, 0, 0);
            }
        }
    }
}

// t of this lane's 8 scores of a chunk and scenario tile: sc[r] / sc[4 + r] the output scales of
// its vertices 4g + r / 16 + 4g + r
__device__ __forceinline__ void i8_chunk_scores(const i4 (&acc)[ci8::kL][2], const float (&sc)[8], f4 &tlo, f4 &thi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int lo[ci8::kL], hi[ci8::kL];
#pragma unroll
        for (int l = 0; l < ci8::kL; ++l) { lo[l] = acc[l][0][r]; hi[l] = acc[l][1][r]; }
        tlo[r] = ci8::combine(lo, sc[r]);
        thi[r] = ci8::combine(hi, sc[4 + r]);
    }
}

#ifndef TWOSD_CUT4_BPC
#define TWOSD_CUT4_BPC 3                 // blocks per CU the integer pass is compiled for
#endif

template <int KB>
__global__ void __launch_bounds__(256, TWOSD_CUT4_BPC) cut_argmax4_kernel(CutParams P) {
    if (*P.mode != 2) return;                       // another pass runs this cut
    constexpr int KS = KB <= 16 ? 1 : 2;            // k-steps of 64 (k <= 64: KB <= 16)
    constexpr int CB = i8_chunk_bytes(KS);
    __shared__ __attribute__((aligned(16))) int8_t Bs[2][CB];   // double-buffered chunk image
    __shared__ double Bb[3][kVT2];                  // the chunks' fp64 bases (ring of 3: finish reads chunk ch - 1)
    extern __shared__ unsigned long long hl[];      // nv entries when P.hist_lds
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (P.hist_lds)
        for (int v = threadIdx.x; v < P.nv; v += 256) hl[v] = 0ull;
    const int g = lane >> 4, j = lane & 15;
    const int nvc = *P.nvc;
    const int nchunks = (nvc + kVT2 - 1) / kVT2;
    const int nunits = cut_num_units(P);
    const double band = cut_band_scalar(P);
    const double rel = P.tie_rel;
    double pv_sum = 0.0;
    double Sacc[2] = {0.0, 0.0};   // lane (g, j): e = 4 kb + g for kb = j, j + 16

    for (int unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const bool tail = unit >= P.full_units;
        const int tile = tail ? P.full_units + (unit - P.full_units) / P.tail_S : unit;
        const int range = tail ? (unit - P.full_units) % P.tail_S : 0;
        const int c_lo = tail ? (int)((long long)nchunks * range / P.tail_S) : 0;
        const int c_hi = tail ? (int)((long long)nchunks * (range + 1) / P.tail_S) : nchunks;
        const int s0 = tile * kCutTile2 + wid * 32;
        const int sa = s0 + j, sb = s0 + 16 + j;
        i4 d0[KS][ci8::kL], d1[KS][ci8::kL];
        i8_quant_deltas<KS>(P, sa, g, d0);
        i8_quant_deltas<KS>(P, sb, g, d1);
        RowEx rb0 = row_ex_init(), rb1 = rb0;
        int *const lbase = tail ? P.tcand : P.cand;
        const unsigned log0 = tail ? (unsigned)(((((size_t)(s0 + j - P.full_units * kCutTile2)) * P.tail_S + range) * 4 + g) * kCandC)
                                      : (unsigned)((((size_t)(s0 + j)) * 4 + g) * kCandC);
        const unsigned lstep = 16u * (tail ? P.tail_S : 1) * 4 * kCandC;

        // LDS-DMA staging: the chunk image is copied as it lies, 1 KiB (64 lanes x 16 bytes) per instruction
        auto stage = [&](int buf, int bslot, int v0) {
            const int8_t *src = P.PKq + (size_t)(v0 / kVT2) * CB;
            for (int i = wid; i < CB / 1024; i += 4)
                __builtin_amdgcn_global_load_lds((const void *)(src + i * 1024 + lane * 16),
                                                 (__attribute__((address_space(3))) void *)&Bs[buf][i * 1024], 16, 0, 0);
            if (wid == 3 && lane < 16)
                __builtin_amdgcn_global_load_lds((const void *)(P.basec + v0 + 2 * lane),
                                                 (__attribute__((address_space(3))) void *)&Bb[bslot][0], 16, 0, 0);
        };
        // this lane's 8 vertices of a chunk: prefilter bases (as v3) and output scales
        auto load_bases = [&](float (&bq)[8], float (&sq)[8], int v0) {
            const f4 lo = *reinterpret_cast<const f4 *>(P.basec32 + v0 + 4 * g);
            const f4 hi = *reinterpret_cast<const f4 *>(P.basec32 + v0 + 16 + 4 * g);
            const f4 slo = *reinterpret_cast<const f4 *>(P.scq + v0 + 4 * g);
            const f4 shi = *reinterpret_cast<const f4 *>(P.scq + v0 + 16 + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) { bq[r] = lo[r]; bq[4 + r] = hi[r]; sq[r] = slo[r]; sq[4 + r] = shi[r]; }
        };
        // v3's finish, a second copy: prefilter in fp32, exact steps in vertex order for the lanes past it.  (As
        // one function -- RowEx &, the four tiles, the base slot -- the chunk loop went from 0 scratch loads
        // / 0 stores to 6 / 4 in the fp32 pass at KB 8 and from 7 / 1 to 8 / 4 here at KB 30.)
        auto finish = [&](const f4 &q00, const f4 &q01, const f4 &q10, const f4 &q11, const float (&bb)[8], int vb, int bslot) {
            unsigned m0 = 0, m1 = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                m0 |= (unsigned)(bb[r] + q00[r] >= rb0.thr32) << r;
                m1 |= (unsigned)(bb[r] + q01[r] >= rb1.thr32) << r;
                m0 |= (unsigned)(bb[4 + r] + q10[r] >= rb0.thr32) << (4 + r);
                m1 |= (unsigned)(bb[4 + r] + q11[r] >= rb1.thr32) << (4 + r);
            }
            while (__builtin_amdgcn_ballot_w64((m0 | m1) != 0) != 0) {
                const int r0 = m0 ? __builtin_ctz(m0) : 0, r1 = m1 ? __builtin_ctz(m1) : 0;
                const int o0 = (r0 >> 2) * 16 + 4 * g + (r0 & 3), o1 = (r1 >> 2) * 16 + 4 * g + (r1 & 3);
                const double b0 = Bb[bslot][o0], b1 = Bb[bslot][o1];
                const float t0 = r0 < 4 ? q00[r0 & 3] : q10[r0 & 3];
                const float t1 = r1 < 4 ? q01[r1 & 3] : q11[r1 & 3];
                const double s0 = (vb + o0 < nvc ? b0 : -INFINITY) + (double)t0;
                const double s1 = (vb + o1 < nvc ? b1 : -INFINITY) + (double)t1;
                if (m0) row_fast<true>(rb0, s0, vb + o0, rel, band, lbase, log0);
                if (m1) row_fast<true>(rb1, s1, vb + o1, rel, band, lbase, log0 + lstep);
                m0 &= m0 - 1;
                m1 &= m1 - 1;
            }
        };
        f4 p[4] = {};
        float bp[8];
        int pv0 = 0;
        stage(0, 0, c_lo * kVT2);
        __syncthreads();
        int bs = 0, bsp = 0;   // base ring slots of chunks ch and ch - 1
        for (int ch = c_lo; ch < c_hi; ++ch) {
            const int buf = (ch - c_lo) & 1;
            const int v0 = ch * kVT2;
            float bq[8], sq[8];
            load_bases(bq, sq, v0);                 // in flight under the MFMAs
            if (ch + 1 < c_hi) stage(buf ^ 1, bs == 2 ? 0 : bs + 1, v0 + kVT2);
            {
                i4 acc[ci8::kL][2] = {};
                i8_chunk_mma<KS>(&Bs[buf][0], g, j, d0, acc);
                if (ch > c_lo) finish(p[0], p[1], p[2], p[3], bp, pv0, bsp);   // the previous chunk, under these MFMAs
                i8_chunk_scores(acc, sq, p[0], p[2]);
            }
            __builtin_amdgcn_sched_barrier(0);
            {
                i4 acc[ci8::kL][2] = {};
                i8_chunk_mma<KS>(&Bs[buf][0], g, j, d1, acc);
                i8_chunk_scores(acc, sq, p[1], p[3]);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) bp[r] = bq[r];
            pv0 = v0;
            bsp = bs;
            bs = bs == 2 ? 0 : bs + 1;
            __syncthreads();
        }
        if (c_hi > c_lo) finish(p[0], p[1], p[2], p[3], bp, pv0, bsp);
        // cut_tile_end<KB, true> (int sources), a second copy: calling it instead -- whole, in halves, or
        // only its pick_terms -- took this chunk loop from 6 scratch accesses per step to 8-15 at KB 24 and
        // 32, and from 1 to 2 at KB 8; only KB 22 and 30 can be timed (ssn, storm)
        int pk0, pk1, nt0, nt1;
        combine_ex(rb0, rel, band, g, pk0, nt0);
        combine_ex(rb1, rel, band, g, pk1, nt1);
        if (rb0.n > 0 && (tail || nt0 >= 2)) lbase[log0] = rb0.f;
        if (rb1.n > 0 && (tail || nt1 >= 2)) lbase[log0 + lstep] = rb1.f;
        rb0.I = rb0.I >= 0 ? P.vmap[rb0.I] : -1;
        rb1.I = rb1.I >= 0 ? P.vmap[rb1.I] : -1;
        if (tail) {
            if (g == 0) {
                const int t0 = P.full_units * kCutTile2;
                if (sa < P.N) {
                    const size_t o = (size_t)(sa - t0) * P.tail_S + range;
                    P.tp_m[o] = rb0.M; P.tp_i[o] = rb0.I; P.tp_f[o] = pk0;
                }
                if (sb < P.N) {
                    const size_t o = (size_t)(sb - t0) * P.tail_S + range;
                    P.tp_m[o] = rb1.M; P.tp_i[o] = rb1.I; P.tp_f[o] = pk1;
                }
            }
            continue;
        }
        if (nt0 < 2) pk0 = 0;
        if (nt1 < 2) pk1 = 0;
        const bool ok0 = sa < P.N && !pk0 && rb0.I >= 0, ok1 = sb < P.N && !pk1 && rb1.I >= 0;
        const double p0 = ok0 ? P.w[sa] * P.inv_total : 0.0, p1 = ok1 ? P.w[sb] * P.inv_total : 0.0;
        // the fp64 deltas again for the S_e terms and the decided rows' values
        auto fin = [&](int sx, bool ok, int ai, double pp) -> double {
            const double *pk = P.PK + (size_t)(ai >= 0 ? ai : 0) * P.k4;
            const double pu = ok ? pp : 0.0;
            constexpr int FG = 6;
            double cg = 0.0;
#pragma unroll
            for (int k0 = 0; k0 < KB; k0 += FG) {
                double d64[FG], pke[FG];
#pragma unroll
                for (int u = 0; u < FG; ++u) {
                    const int e = 4 * (k0 + u) + g;
                    const bool in = k0 + u < KB && e < P.k;
                    d64[u] = (in && sx < P.N) ? P.dv[(size_t)sx * P.k + e] : 0.0;
                    pke[u] = in ? pk[e] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < FG; ++u) {
                    const int kb = k0 + u, e = 4 * kb + g;
                    if (kb >= KB) break;
                    if (e < P.k) cg = fma(pke[u] * P.coef[e], d64[u], cg);
                    double v = (e < P.k) ? pu * pke[u] * d64[u] : 0.0;
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
                    if (j == (kb & 15)) {
                        if (kb < 16) Sacc[0] += v;
                        else Sacc[1] += v;
                    }
                }
            }
            return dec_combine(cg);
        };
        const double tv0 = fin(sa, ok0, rb0.I, p0);
        const double tv1 = fin(sb, ok1, rb1.I, p1);
        const double vl0 = ok0 ? P.base[rb0.I] + tv0 : rb0.M, vl1 = ok1 ? P.base[rb1.I] + tv1 : rb1.M;
        if (g == 0) {
            if (sa < P.N) { P.arg[sa] = rb0.I; P.val[sa] = vl0; P.flag[sa] = pk0; }
            if (sb < P.N) { P.arg[sb] = rb1.I; P.val[sb] = vl1; P.flag[sb] = pk1; }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const int ok = __shfl(t == 0 ? (int)ok0 : (int)ok1, jj);
                const int ai = __shfl(t == 0 ? rb0.I : rb1.I, jj);
                const double pp = __shfl(t == 0 ? p0 : p1, jj);
                const double vl = __shfl(t == 0 ? vl0 : vl1, jj);
                if (lane == 0 && ok) {
                    pv_sum = fma(pp, vl, pv_sum);
                    const unsigned long long hq = (unsigned long long)__double2ull_rn(pp * kFix);
                    if (P.hist_lds) __hip_atomic_fetch_add(&hl[ai], hq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    else atomicAdd(&P.hist[ai], hq);
                }
            }
        }
    }
    if (P.hist_lds) {
        __syncthreads();
        for (int v = threadIdx.x; v < P.nv; v += 256) P.hist_part[(size_t)blockIdx.x * P.nv + v] = hl[v];
    }
    const int slot = blockIdx.x * 4 + wid;
    double *out = P.partial + (size_t)slot * (P.k + 1);
    if (lane == 0) out[0] = pv_sum;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int e = 4 * (j + 16 * t) + g;
        if (e < P.k) out[1 + e] = Sacc[t];
    }
}

// diagnostics: the integer pass's t of every (scenario, compacted vertex), out[s * nvc + c], by the
// device functions of cut_argmax4_kernel (the chunk images read from global memory)
template <int KS>
__global__ void __launch_bounds__(256) cut_scores4_kernel(CutParams P, float *__restrict__ out) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int g = lane >> 4, j = lane & 15;
    const int nvc = *P.nvc;
    const int nchunks = (nvc + kVT2 - 1) / kVT2;
    const int s0 = blockIdx.x * kCutTile2 + wid * 32;
    const int sa = s0 + j, sb = s0 + 16 + j;
    i4 d0[KS][ci8::kL], d1[KS][ci8::kL];
    i8_quant_deltas<KS>(P, sa, g, d0);
    i8_quant_deltas<KS>(P, sb, g, d1);
    for (int ch = 0; ch < nchunks; ++ch) {
        const int v0 = ch * kVT2;
        float sq[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) { sq[r] = P.scq[v0 + 4 * g + r]; sq[4 + r] = P.scq[v0 + 16 + 4 * g + r]; }
        f4 t[4];
        for (int st = 0; st < 2; ++st) {
            i4 acc[ci8::kL][2] = {};
            i8_chunk_mma<KS>(P.PKq + (size_t)ch * i8_chunk_bytes(KS), g, j, st ? d1 : d0, acc);
            i8_chunk_scores(acc, sq, t[st], t[2 + st]);
        }
#pragma unroll
        for (int tile = 0; tile < 4; ++tile)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = v0 + (tile >> 1) * 16 + 4 * g + r, s = (tile & 1) ? sb : sa;
                if (c < nvc && s < P.N) out[(size_t)s * nvc + c] = t[tile][r];
            }
    }
}

// hist[v] += sum over blocks of the block histograms (integers: exact in any order)
__global__ void __launch_bounds__(256) cut_hist_reduce_kernel(int nb, int nv, const unsigned long long *__restrict__ part,
                                                              unsigned long long *__restrict__ hist) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    unsigned long long s = 0;
    for (int b = 0; b < nb; ++b) s += part[(size_t)b * nv + v];
    hist[v] += s;
}

// the argmax kernel of (pass, KB); pass as band_bits[BAND_PASS] has it: 0 fp64, 1 fp32, 2 integer
typedef void (*cut_argmax_fn)(CutParams);
template <size_t... I>
static cut_argmax_fn argmax_kernel_of(int pass, int KB, std::index_sequence<I...>) {
    static const cut_argmax_fn tab[3][kNumKB] = {{cut_argmax2_kernel<kCutKBs[I]>...},
                                                 {cut_argmax3_kernel<kCutKBs[I]>...},
                                                 {cut_argmax4_kernel<kCutKBs[I]>...}};
    for (int i = 0; i < kNumKB; ++i)
        if (kCutKBs[i] == KB) return tab[pass][i];
    return nullptr;
}
static cut_argmax_fn argmax_kernel(int pass, int KB) { return argmax_kernel_of(pass, KB, std::make_index_sequence<kNumKB>{}); }

// resident blocks per CU of one instantiation (registers and LDS): the persistent grid is
// sized to exactly what is resident, so no block starts after the first ones drain (a grid
// of 3 blocks per CU at 2 resident ran its last third with half of every CU idle)
static int argmax_occupancy(cut_argmax_fn fn, size_t dyn_lds) {
    int nb = 0;
    if (!fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 256, dyn_lds) != hipSuccess) nb = 0;
    return nb;
}

static void launch_argmax(cut_argmax_fn fn, const CutParams &P, int nblocks, hipStream_t s) {
    hipLaunchKernelGGL(fn, dim3(nblocks), dim3(256), P.hist_lds ? sizeof(unsigned long long) * P.nv : 0, s, P);
}

int cut_argmax_bpc(int k, const CutKnobs &kn) {
    CutPlan pl;
    int bpc = kn.bpc;
    // blocks per CU: resident occupancy of this instantiation (TWOSD_CUT_BPC overrides; the
    // |V| <= kHistLds case adds the LDS histogram, at most 2 KB)
    if (bpc <= 0 && cut_plan_passes(k, kn, kCutKBs, kNumKB, pl))
        bpc = argmax_occupancy(pl.wanti8 ? argmax_kernel(2, pl.KB32) : pl.want32 ? argmax_kernel(1, pl.KB32) : argmax_kernel(0, pl.KB),
                               sizeof(unsigned long long) * kHistLds);
    return bpc <= 0 ? 2 : bpc;
}

void cut_argmax_stage(const CutPlan &pl, const CutParams &P, hipStream_t s) {
    if (pl.wanti8) launch_argmax(argmax_kernel(2, pl.KB32), P, pl.nblocks, s);   // each of the three returns at once unless its pass runs
    if (pl.want32) launch_argmax(argmax_kernel(1, pl.KB32), P, pl.nblocks, s);
    launch_argmax(argmax_kernel(0, pl.KB), P, pl.nblocks, s);
    if (P.hist_lds)
        hipLaunchKernelGGL(cut_hist_reduce_kernel, dim3((P.nv + 255) / 256), dim3(256), 0, s, pl.nblocks, P.nv, P.hist_part, P.hist);
}

void cut_scores_stage(const CutPlan &pl, const CutParams &P, int KS, float *d_out, hipStream_t s) {
    if (KS == 1) hipLaunchKernelGGL(cut_scores4_kernel<1>, dim3(pl.ntiles), dim3(256), 0, s, P, d_out);
    else hipLaunchKernelGGL(cut_scores4_kernel<2>, dim3(pl.ntiles), dim3(256), 0, s, P, d_out);
}

}  // namespace twosd
