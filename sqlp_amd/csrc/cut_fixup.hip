// cut_fixup.hip -- after the argmax passes (the maths: cut_kernel.hip): the tail ranges' merge, the
// re-decision of the rows with several vertices in the band in the restatement's arithmetic, and
// the full re-scan of the rows whose candidate log overflowed.
#include <hip/hip_runtime.h>
#include <math.h>
#include "cut_common.h"

namespace twosd {

// Tail scenarios: merge the per-range results -- the same rule as combine_ex over the ranges:
// M = max, a range contributes its log lengths when its maximum reaches the band of M; one
// entry in all: decided (the pick is that range's first maximum), then the scenario's p * val,
// histogram weight and S_e terms (as cut_fixup_kernel); several: flag for the fixup (val = M).
// One wavefront per scenario, lane r = range r.
__device__ __forceinline__ int nib_sum(int pk) {
    return (pk & 31) + ((pk >> kCandBits) & 31) + ((pk >> (2 * kCandBits)) & 31) + ((pk >> (3 * kCandBits)) & 31);
}

__global__ void __launch_bounds__(256) cut_tail_merge_kernel(CutParams P, int slot0) {
    const int lane = threadIdx.x & 63;
    const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nw = (gridDim.x * blockDim.x) >> 6;
    const int t0 = P.full_units * kCutTile2, S = P.tail_S;
    const double band = __longlong_as_double((long long)*P.band_bits);
    double pv_sum = 0.0, Sacc[2] = {0.0, 0.0};
    for (int ts = gw; ts < P.N - t0; ts += nw) {
        const int s = t0 + ts;
        double m = -INFINITY;
        int ii = -1, pk = 0;
        if (lane < S) {
            const size_t o = (size_t)ts * S + lane;
            m = P.tp_m[o]; ii = P.tp_i[o]; pk = P.tp_f[o];
        }
        double M = m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) M = fmax(M, __shfl_xor(M, o));
        const double thr = band_floor(M, P.tie_rel, band);
        const int n = (m != -INFINITY && m >= thr) ? nib_sum(pk) : 0;
        int tot = n, it = n ? ii : 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            tot += __shfl_xor(tot, o);
            it = min(it, __shfl_xor(it, o));
        }
        const int I = (M == -INFINITY || it == 0x7fffffff) ? -1 : it;
        const int fl = tot >= 2;
        if (lane == 0) { P.arg[s] = I; P.val[s] = M; P.flag[s] = fl; }
        if (fl || I < 0) continue;
        const double p = P.w[s] * P.inv_total;
        // the S_e terms of the pick and its value in fp64, base[I] + sum_e PK[I,e] coef_e dv_e (the
        // lanes' terms summed by a fixed xor tree; the pass's maximum M may be an fp32-MFMA score)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int e = lane + 64 * t;
            if (e < P.k) Sacc[t] = fma(p * P.PK[(size_t)I * P.k4 + e], P.dv[(size_t)s * P.k + e], Sacc[t]);
        }
        // lane g < 4: the chain c_g of cut_tile_end's pick_terms, then (c_0 + c_1) + (c_2 + c_3) as dec_combine
        double cg = 0.0;
        if (lane < 4) {
            const double *pk = P.PK + (size_t)I * P.k4, *dr = P.dv + (size_t)s * P.k;
            for (int e = lane; e < P.k; e += 4) cg = fma(pk[e] * P.coef[e], dr[e], cg);
        }
        const double c01 = __shfl(cg, 0) + __shfl(cg, 1), c23 = __shfl(cg, 2) + __shfl(cg, 3);
        const double vl = P.base[I] + (c01 + c23);
        if (lane == 0) {
            P.val[s] = vl;
            pv_sum = fma(p, vl, pv_sum);
            atomicAdd(&P.hist[I], (unsigned long long)__double2ull_rn(p * kFix));
        }
    }
    double *out = P.partial + (size_t)(slot0 + gw) * (P.k + 1);
    if (lane == 0) out[0] = pv_sum;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int e = lane + 64 * t;
        if (e < P.k) out[1 + e] = Sacc[t];
    }
}

// score[s, v] in the restatement's order (oracle_build_cut, twosd_ref.argmax_procedure):
// t = sum over the random rows in ascending order of pi_v[row_e] (coef_e dv[s,e]) -- the dense
// dot(pi, dvec) of subprob.jl:155 with its zero rows dropped (adding 0 is exact) -- every
// operation rounded on its own, then base[v] + t
__device__ __forceinline__ double restated_score(const CutParams &P, int v, int s) {
#pragma clang fp contract(off)
    const double *po = P.PKO + (size_t)v * P.k4;
    const double *d = P.dv + (size_t)s * P.k;
    double t = 0.0;
#pragma unroll 4
    for (int q = 0; q < P.k; ++q) {
        const int e = P.eord[q];
        t = t + po[q] * (P.coef[e] * d[e]);
    }
    return P.base[v] + t;
}

// Re-decide the flagged scenarios in the restatement's arithmetic: the logged candidates of the
// lane groups (and tail ranges) that reach the band hold every vertex that can be the pick.
// tie_rel = 0: the first strict maximum (highest score, lowest index among equal scores); > 0:
// the lowest index within tie_rel (1 + |M|) of the maximum M (oracle_build_cut's rule).
// Rows go in batches of up to kFxR flagged whole-tile scenarios per wavefront (a tail scenario,
// whose logs span the vertex ranges, is a batch of its own), so every memory round trip of a
// batch -- the flags, the logs, the staged deltas, the candidates' PK rows, the sums -- serves
// all of its rows:
//   1. the rows' coef_e dv[s,e] in the restated element order (eord) into LDS (dvr);
//   2. the logged candidates compacted into one LDS list, row by row (slot order);
//   3. one lane per candidate adds its products pi_v[row_e] dvr[q] in order (the sequential
//      chain of restated_score; the PK gathers are independent of it and run ahead);
//   4. lane r decides row r over its candidates; then the sums of the decided rows.
// A log that overflowed (or a list past kFxList) re-scans every vertex for that row.
constexpr int kFxR = 8;              // flagged scenarios per batch
constexpr int kFxLd = 129;           // doubles per staged delta row (k <= 128; odd stride)
constexpr int kFxList = 256;         // candidate list capacity per batch (8 rows x 32 log slots)

struct FixWave {                     // one wavefront's LDS
    double dvr[kFxR][kFxLd];
    double cs[kFxList];
    int cvr[kFxList];                // (row << 28) | vertex
};

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// t = sum_q PKO[v][q] wq[q] in q order, wq[q] = cq[q] dq[q] (the restated k-term dot of one
// candidate; the products past k are 0 and leave t unchanged: t is never -0).  The PKO row is read
// in groups of 32 elements (16 dwordx4 loads), the next group's loads issued before this group's adds.
__device__ __forceinline__ double chain_dot_w(const double2 *__restrict__ po, const double *wq, int k4) {
#pragma clang fp contract(off)
    constexpr int GQ = 8;    // pairs per group (16 elements); k4 <= 128: at most 8 groups
    const int k2 = k4 / 2;
    double t = 0.0;
    double2 a[GQ], b[GQ];
    auto load = [&](double2 (&x)[GQ], int g) {
#pragma unroll
        for (int u = 0; u < GQ; ++u) {
            const int pu = g * GQ + u;
            const double2 ld = po[pu < k2 ? pu : k2 - 1];
            x[u] = pu < k2 ? ld : make_double2(0.0, 0.0);
        }
    };
    auto add = [&](const double2 (&x)[GQ], int g) {
#pragma unroll
        for (int u = 0; u < GQ; ++u) {
            const int q = 2 * (g * GQ + u);
            if (q < k4) {   // uniform
                t = t + x[u].x * wq[q];
                t = t + x[u].y * wq[q + 1];
            }
        }
    };
    const int ng = (k2 + GQ - 1) / GQ;
    load(a, 0);
    for (int g = 0; g < ng; g += 2) {   // ping-pong: group g + 1 in flight while g is added
        if (g + 1 < ng) load(b, g + 1);
        add(a, g);
        if (g + 1 >= ng) break;
        if (g + 2 < ng) load(a, g + 2);
        add(b, g + 1);
    }
    return t;
}

// chain_dot_w with the products cq[q] dq[q] formed in the loop (the rescan's one-row form)
__device__ __forceinline__ double chain_dot(const double2 *__restrict__ po, const double *cq, const double *dq, int k4) {
#pragma clang fp contract(off)
    constexpr int GQ = 8;    // pairs per group (16 elements); k4 <= 128: at most 8 groups
    const int k2 = k4 / 2;
    double t = 0.0;
    double2 a[GQ], b[GQ];
    auto load = [&](double2 (&x)[GQ], int g) {
#pragma unroll
        for (int u = 0; u < GQ; ++u) {
            const int pu = g * GQ + u;
            const double2 ld = po[pu < k2 ? pu : k2 - 1];
            x[u] = pu < k2 ? ld : make_double2(0.0, 0.0);
        }
    };
    auto add = [&](const double2 (&x)[GQ], int g) {
#pragma unroll
        for (int u = 0; u < GQ; ++u) {
            const int q = 2 * (g * GQ + u);
            if (q < k4) {   // uniform
                t = t + x[u].x * (cq[q] * dq[q]);
                t = t + x[u].y * (cq[q + 1] * dq[q + 1]);
            }
        }
    };
    const int ng = (k2 + GQ - 1) / GQ;
    load(a, 0);
    for (int g = 0; g < ng; g += 2) {   // ping-pong: group g + 1 in flight while g is added
        if (g + 1 < ng) load(b, g + 1);
        add(a, g);
        if (g + 1 >= ng) break;
        if (g + 2 < ng) load(a, g + 2);
        add(b, g + 1);
    }
    return t;
}

constexpr int kFlagRescan = 0x40000000;   // flag of a scenario left to cut_rescan_kernel (an overflowed log)

__global__ void __launch_bounds__(256, 3) cut_fixup_kernel(CutParams P, int slot0) {
#pragma clang fp contract(off)
    __shared__ FixWave fw_all[4];
    __shared__ double cq[kFxLd];             // coef_e in the restated order (0 past k)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    FixWave &F = fw_all[wid];
    const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nw = (gridDim.x * blockDim.x) >> 6;
    const int t0 = P.full_units * kCutTile2, S = P.tail_S;
    const double band = cut_band_scalar(P);
    // this lane's elements in the restated order: q = lane, lane + 64 (-1: padding)
    const int e0 = lane < P.k ? P.eord[lane] : -1, e1 = lane + 64 < P.k ? P.eord[lane + 64] : -1;
    if (threadIdx.x < kFxLd) {
        const int q = threadIdx.x;
        cq[q] = q < P.k ? P.coef[P.eord[q]] : 0.0;
    }
    __syncthreads();
    double pv_sum = 0.0, Sq[2] = {0.0, 0.0};  // S_e of this wave in the restated order: q = lane, lane + 64
    unsigned long long st_rows = 0, st_cands = 0, st_full = 0;
#ifdef TWOSD_FIX_STAMPS
    unsigned long long fst[6] = {0, 0, 0, 0, 0, 0}, fst_t = __builtin_amdgcn_s_memtime();
#define FSTAMP(i) { __builtin_amdgcn_s_waitcnt(0); __builtin_amdgcn_sched_barrier(0); \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); fst[i] += t_ - fst_t; fst_t = t_; }
#else
#define FSTAMP(i)
#endif
    // pass 0: the whole-tile rows, 64 consecutive scenarios per wave step; pass 1: the tail rows
    // (each a batch of its own), spread over all waves (lane L of wave gw: scenario t0 + gw + L nw)
    // so that the waves holding the last scenarios do not run one serial batch per tail row
    for (int pass = 0; pass < 2; ++pass) {
    const int hi = pass ? P.N : min(t0, P.N), lstride = pass ? nw : 1;
    const int gs = pass ? 64 : P.fx_gs;     // a small batch: fewer scenarios per wave step, more waves
    for (int sb0 = pass ? t0 + gw : gw * gs; sb0 < hi; sb0 += nw * gs) {
    const int sl = sb0 + lane * lstride;
    const int myflag = (lane < gs && sl < hi) ? P.flag[sl] : 0;
    uint64_t todo = __ballot(myflag != 0);
    while (todo) {
        // ---- the batch: up to kFxR whole-tile rows, or one tail row
        int nr = 0, srow = 0, frow = 0;     // lane r < nr: its row's scenario and flag
        bool tailb = false;
        while (todo && nr < kFxR) {
            const int bit = (int)__builtin_ctzll(todo);
            const int s = sb0 + bit * lstride;
            if (s >= t0) {                       // a tail row: alone in its batch
                if (nr > 0) break;
                tailb = true;
            }
            todo &= todo - 1;
            const int fl = __shfl(myflag, bit);
            if (lane == nr) { srow = s; frow = fl; }
            ++nr;
            if (tailb) break;
        }
        FSTAMP(0)
        // 1. the rows' deltas in the restated order, all loads in one round trip: the products
        // coef_e dv_e of the restated dot into LDS (zero past k; the same operation the chain would
        // do), the raw deltas kept in registers for the S_e sums
        double d0[kFxR], d1[kFxR];
        {
#pragma unroll
            for (int r = 0; r < kFxR; ++r) {
                const int s = __shfl(srow, r < nr ? r : 0);
                const double *dr = P.dv + (size_t)s * P.k;
                d0[r] = e0 >= 0 ? dr[e0] : 0.0;
                d1[r] = e1 >= 0 ? dr[e1] : 0.0;
            }
            const double c0 = cq[lane], c1 = cq[lane + 64];
#pragma unroll
            for (int r = 0; r < kFxR; ++r) {
                if (r < nr) {
                    F.dvr[r][lane] = c0 * d0[r];
                    F.dvr[r][lane + 64] = c1 * d1[r];
                }
            }
        }
        FSTAMP(1)
        // 2. the candidate list (slot order: rows in batch order, each row's slots contiguous)
        int nc = 0;
        uint32_t rstart = 0, rcount = 0;        // lane r: its row's list range
        uint32_t ovf_rows = 0;                  // rows whose log overflowed (or a list past kFxList)
        if (!tailb) {
            constexpr int NIT = kFxR;         // one step per row (4 kCandC == 64 slots)
            int vv[NIT];
#pragma unroll
            for (int it = 0; it < NIT; ++it) {   // every log entry of the batch in one round trip
                const int g = lane / kCandC, i = lane % kCandC;
                const int fl = __shfl(frow, it);
                const int sr = __shfl(srow, it);
                const int c = (fl >> (kCandBits * g)) & 31;
                const int lv = P.cand[((size_t)sr * 4 + g) * kCandC + i];   // rows past nr: srow = 0, a valid address
                vv[it] = it >= nr ? -1 : (c > kCandC ? -2 : (i < c ? lv : -1));   // log entries: argmax positions (vmap)
            }
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                if (it >= nr) break;
                const int v = vv[it];
                const uint64_t has = __ballot(v >= 0);
                const int na = __popcll(has);
                if (__ballot(v == -2) != 0 || nc + na > kFxList) {   // overflowed log (or a full list): rescan
                    ovf_rows |= 1u << it;
                    continue;
                }
                if (v >= 0) F.cvr[nc + __popcll(has & ((1ull << lane) - 1))] = (it << 28) | v;
                if (lane == it) { rstart = nc; rcount = na; }
                nc += na;
            }
        } else {
            const int s = __shfl(srow, 0);
            const int ts = s - t0;
            const double thr = band_floor(P.val[s], P.tie_rel, band);
            const int nslots = S * 4 * kCandC;
            for (int q0 = 0; q0 < nslots; q0 += 64) {
                const int q = q0 + lane;
                int v = -1;
                if (q < nslots) {
                    const int rg = q / (4 * kCandC), g = (q / kCandC) & 3, i = q % kCandC;
                    const size_t o = (size_t)ts * S + rg;
                    const double mr = P.tp_m[o];
                    const int pk = (mr != -INFINITY && mr >= thr) ? P.tp_f[o] : 0;
                    const int c = (pk >> (kCandBits * g)) & 31;
                    if (c > kCandC) v = -2;
                    else if (i < c) v = P.tcand[(o * 4 + g) * kCandC + i];
                }
                const uint64_t has = __ballot(v >= 0);
                if (__ballot(v == -2)) ovf_rows = 1u;
                if (nc + __popcll(has) > kFxList) { ovf_rows = 1u; break; }
                if (v >= 0) F.cvr[nc + __popcll(has & ((1ull << lane) - 1))] = v;
                nc += __popcll(has);
            }
            if (lane == 0) { rstart = 0; rcount = nc; }
        }
        wave_lds_sync();
        FSTAMP(2)
        st_rows += nr;
        st_cands += nc;
        // 3. restated scores, one lane per candidate: base[v] + chain_dot (restated_score's order);
        // candidates are argmax positions (vertex vmap[c]: PKOc / basec rows)
        for (int cb = 0; cb < nc; cb += 64) {
            const int c = cb + lane;
            const int cr = F.cvr[c < nc ? c : 0];
            const int r = cr >> 28, v = cr & 0x0fffffff;
            const double bvv = P.basec[v];
            const double t = chain_dot_w(reinterpret_cast<const double2 *>(P.PKOc + (size_t)v * P.k4), F.dvr[r], P.k4);
            if (c < nc) F.cs[c] = bvv + t;
        }
        wave_lds_sync();
        FSTAMP(3)
        // 4. lane r decides row r over its candidates (the rule takes the lowest vertex among the
        // qualifying ones, whatever their list order; positions order as the vertices)
        int best = 0x7fffffff;
        double bv = -INFINITY;
        if (lane < nr && !((ovf_rows >> lane) & 1)) {
            double M = -INFINITY;
            for (uint32_t c = rstart; c < rstart + rcount; ++c) M = fmax(M, F.cs[c]);
            if (M != -INFINITY) {
                const double lim = P.tie_rel > 0.0 ? M - P.tie_rel * (1.0 + fabs(M)) : M;
                for (uint32_t c = rstart; c < rstart + rcount; ++c) {
                    const int v = F.cvr[c] & 0x0fffffff;
                    const double sc = F.cs[c];
                    if (sc >= lim && v < best) { best = v; bv = sc; }
                }
            }
        }
        // overflowed rows: left to cut_rescan_kernel (every vertex), which also adds their sums
        const bool resc = lane < nr && ((ovf_rows >> lane) & 1);
        if (resc) P.flag[srow] = kFlagRescan;
        st_full += __popc(ovf_rows);
        FSTAMP(4)
        // 5. outputs and sums, rows in batch (= scenario) order; the picks' vertex indices and PKO
        // rows in one round trip
        const bool mine = lane < nr && best != 0x7fffffff;
        const int bvx = mine ? P.vmap[best] : -1;
        {
            double pa[kFxR], pb[kFxR];
#pragma unroll
            for (int r = 0; r < kFxR; ++r) {
                const int b = __shfl(best, r < nr ? r : 0);
                const double *po = P.PKOc + (size_t)(b == 0x7fffffff ? 0 : b) * P.k4;
                pa[r] = po[lane < P.k4 ? lane : 0];
                pb[r] = po[lane + 64 < P.k4 ? lane + 64 : 0];
            }
            // lane r: its row's p and histogram weight (one load, one atomic instruction for all rows)
            const double pr = lane < nr ? P.w[srow] * P.inv_total : 0.0;
            if (lane < nr && !resc) {
                P.arg[srow] = bvx;
                P.val[srow] = mine ? bv : -INFINITY;
            }
            if (mine) atomicAdd(&P.hist[bvx], (unsigned long long)__double2ull_rn(pr * kFix));
#pragma unroll
            for (int r = 0; r < kFxR; ++r) {
                if (r >= nr) break;
                const int b = __shfl(best, r);
                const double bvr = __shfl(bv, r);
                const double p = __shfl(pr, r);
                if (b == 0x7fffffff) continue;   // no finite score: no pick (as the argmax pass leaves it)
                if (lane == 0) pv_sum = fma(p, bvr, pv_sum);
                if (e0 >= 0) Sq[0] = fma(p * pa[r], d0[r], Sq[0]);
                if (e1 >= 0) Sq[1] = fma(p * pb[r], d1[r], Sq[1]);
            }
        }
        wave_lds_sync();   // the next batch rewrites the LDS lists
        FSTAMP(5)
    }
    }
    }
    double *out = P.partial + (size_t)(slot0 + gw) * (P.k + 1);
    if (lane == 0) out[0] = pv_sum;
    if (e0 >= 0) out[1 + e0] = Sq[0];
    if (e1 >= 0) out[1 + e1] = Sq[1];
    if (P.fstats && lane == 0 && st_rows) {
        atomicAdd(&P.fstats[CS_FIX_ROWS], st_rows);
        atomicAdd(&P.fstats[CS_FIX_CANDS], st_cands);
        atomicAdd(&P.fstats[CS_FIX_RESCANS], st_full);
#ifdef TWOSD_FIX_STAMPS
        for (int i_ = 0; i_ < CS_FIX_STAMPS; ++i_) atomicAdd(&P.fstats[CS_FIX_STAMP0 + i_], fst[i_]);
#endif
    }
}

// The scenarios whose candidate log overflowed (cut_fixup_kernel marked them kFlagRescan): the
// restated rule over EVERY vertex, one wavefront per scenario, lanes taking the vertices in
// increasing order (64 per step) with chain_dot; pass 0 the first strict maximum, pass 1
// (tie_rel > 0) the lowest vertex within the tolerance.  Then the scenario's sums, as the fixup.
__global__ void __launch_bounds__(256) cut_rescan_kernel(CutParams P, int slot0) {
#pragma clang fp contract(off)
    __shared__ double dqs[4][kFxLd];
    __shared__ double cq[kFxLd];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    double *dq = dqs[wid];
    const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nw = (gridDim.x * blockDim.x) >> 6;
    const int e0 = lane < P.k ? P.eord[lane] : -1, e1 = lane + 64 < P.k ? P.eord[lane + 64] : -1;
    if (threadIdx.x < kFxLd) {
        const int q = threadIdx.x;
        cq[q] = q < P.k ? P.coef[P.eord[q]] : 0.0;
    }
    __syncthreads();
    double pv_sum = 0.0, Sq[2] = {0.0, 0.0};
    for (int sb0 = gw * 64; sb0 < P.N; sb0 += nw * 64) {
    uint64_t todo = __ballot(sb0 + lane < P.N && P.flag[sb0 + lane] == kFlagRescan);
    while (todo) {
        const int s = sb0 + (int)__builtin_ctzll(todo);
        todo &= todo - 1;
        const double *dr = P.dv + (size_t)s * P.k;
        dq[lane] = e0 >= 0 ? dr[e0] : 0.0;
        dq[lane + 64] = e1 >= 0 ? dr[e1] : 0.0;
        wave_lds_sync();
        double bm = -INFINITY;
        int bi = 0x7fffffff;
        for (int v0 = 0; v0 < P.nv; v0 += 64) {
            const int v = v0 + lane;
            const int vc = v < P.nv ? v : P.nv - 1;
            const double sc = P.base[vc] + chain_dot(reinterpret_cast<const double2 *>(P.PKO + (size_t)vc * P.k4), cq, dq, P.k4);
            if (v < P.nv && sc > bm) { bm = sc; bi = v; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double m2 = __shfl_xor(bm, o);
            const int i2 = __shfl_xor(bi, o);
            if (m2 > bm || (m2 == bm && i2 < bi)) { bm = m2; bi = i2; }
        }
        int best = bi;
        double bv = bm;
        if (P.tie_rel > 0.0 && best != 0x7fffffff) {
            const double lim = bm - P.tie_rel * (1.0 + fabs(bm));
            int lo = 0x7fffffff;
            double lv = -INFINITY;
            for (int v0 = 0; v0 < best; v0 += 64) {
                const int v = v0 + lane;
                const int vc = v < P.nv ? v : P.nv - 1;
                const double sc = P.base[vc] + chain_dot(reinterpret_cast<const double2 *>(P.PKO + (size_t)vc * P.k4), cq, dq, P.k4);
                if (v < best && sc >= lim && v < lo) { lo = v; lv = sc; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const int i2 = __shfl_xor(lo, o);
                const double v2 = __shfl_xor(lv, o);
                if (i2 < lo) { lo = i2; lv = v2; }
            }
            if (lo < best) { best = lo; bv = lv; }
        }
        if (lane == 0) {
            P.arg[s] = best == 0x7fffffff ? -1 : best;
            P.val[s] = best == 0x7fffffff ? -INFINITY : bv;
        }
        if (best != 0x7fffffff) {
            const double p = P.w[s] * P.inv_total;
            const double *po = P.PKO + (size_t)best * P.k4;
            if (lane == 0) {
                pv_sum = fma(p, bv, pv_sum);
                atomicAdd(&P.hist[best], (unsigned long long)__double2ull_rn(p * kFix));
            }
            if (e0 >= 0) Sq[0] = fma(p * po[lane], dq[lane], Sq[0]);
            if (e1 >= 0) Sq[1] = fma(p * po[lane + 64], dq[lane + 64], Sq[1]);
        }
        wave_lds_sync();
    }
    }
    double *out = P.partial + (size_t)(slot0 + gw) * (P.k + 1);
    if (lane == 0) out[0] = pv_sum;
    if (e0 >= 0) out[1 + e0] = Sq[0];
    if (e1 >= 0) out[1 + e1] = Sq[1];
}

void cut_fixup_stage(const CutPlan &pl, const CutParams &P, hipStream_t s) {
    if (pl.merge_blocks) hipLaunchKernelGGL(cut_tail_merge_kernel, dim3(pl.merge_blocks), dim3(256), 0, s, P, pl.slot_merge);
    hipLaunchKernelGGL(cut_fixup_kernel, dim3(pl.fix_blocks), dim3(256), 0, s, P, pl.slot_fix);
    hipLaunchKernelGGL(cut_rescan_kernel, dim3(pl.resc_blocks), dim3(256), 0, s, P, pl.slot_rescan);
}

}  // namespace twosd
