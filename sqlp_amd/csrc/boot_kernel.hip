// boot_kernel.hip -- the in-sample stopping rule's device part: stored argmax picks and the
// bootstrap re-formation of cuts from them on gfx950.
//
// Reference: none.  yhz0/SQLP lists "Need to implement stopping criteria" in its readme and
// src/sd_algorithm/plugin/stopping_rule.jl is an empty file.  The rule built here is SD's own
// (Higle and Sen; Sen and Liu 2016): resample the observations, re-form every cut of the master
// from the argmax picks it was built with, and look at the gap at the incumbent.
//
// A cut is linear in the scenario weights once its picks a(s) are fixed (cut_finalize_impl):
//     g = sum_s p_s pi_a(s),  alpha = g.r + sum_{e rhs} S_e (+ c0),  beta = -T'g - sum_{e in T} S_e e_col(e)
//     S_e = sum_s p_s PK[a(s), e] dv[s, e]
// Replicate b weighs scenario s (global index g = index_offset + s) by c_b(g) w_s with
// c_b(g) ~ Poisson(1), a pure function of (seed, g, b): Philox4x32-10, counter (g_lo, g_hi, b >> 2, 1),
// key (seed_lo, seed_hi), word b & 3 through the 12 thresholds of the Poisson(1) CDF.  Row 0 of every
// output is the identity replicate (all counts 1), row 1 + b is replicate b.  Each sum is normalised
// by the replicate's own total W_jb = sum_{s < N_j} c_b w_s, so independent counts (no atomics on
// floating point, the same draws under any sharding) serve where the literature resamples a
// multinomial.
//
// Weights are integers: q_s = rn(w_s 2^58 / total_weight) (total_weight: the caller's global total,
// the same on every rank), so sum_s c q_s <= 12 * 2^58 < 2^62 is exact in uint64 and independent of
// the order of its terms: the per-vertex weights, W_jb and the epigraph totals are bit-identical on
// every run and add exactly across ranks.  The S_e sums are fp64 with a fixed shard layout.
//
// On an epigraph filled from a variance-reduced stream (twosd_sampling, group G) the observations
// are the groups: the _vr entry points give scenario s the count c_b((index_offset + s) / G) of its
// global group index, every member of a group the same, each with its own q_s.  The kernels that
// draw counts are templates: <false> / <KE, 0> are the i.i.d. kernels, the others index their draws
// by the group (boot_index); the host divides index_offset by G once.
//
// Kernels:
//   boot_counts_kernel   the counts themselves (diagnostic: twosd_bootstrap_counts)
//   boot_weight_kernel   sum_{s < n} c_b(s) q_s per replicate (W_jb with n = N_j; the totals with n = N)
//   boot_hist_kernel     the per-vertex weights (M + 1 per pick) as uint64 block histograms in LDS
//                        (windows of 2048 vertices x one Philox call of 4 replicates = 64 KB), flushed
//                        with integer atomics
//   boot_reform_kernel   streams the epigraph's N x k deltas once per replicate group of 16: a wave
//                        walks tiles of 64 scenarios; lanes = scenarios for the Philox draws, then
//                        lanes = elements (e = lane, lane + 64) while the tile's scenarios go by one
//                        at a time with wave-uniform picks and counts (v_readlane); 16 + 1
//                        accumulators per element stay in VGPRs (KE = 2: 191 VGPRs, no scratch)
//   <..., LIST = true>   the three above instantiated over a tail handle's compact list (twosd_tail_keep,
//                        risk.hip: the nt scenarios of a cut scoring above eta, and their picks): the
//                        counts are c_b(s) 1[s in the tail], still a function of the scenario's global
//                        index (or group); only the tail's rows of the deltas are read, in
//                        reform_shards(nt) shards.  Nothing is launched over an empty list (the zero cut).
// then reform.hip's stage, shared with the tail cut of risk.hip: S from the shards' partials, g, and
// alpha, beta per (handle, replicate) normalised by W_jb.  The rule for changing one of these bodies,
// and why risk.hip's look-alikes stay separate kernels: reform.hip's header.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include "reform.h"
#include "philox.h"

namespace twosd {

constexpr int kBootMaxM = 64;            // bootstrap replicates per call
constexpr int kBootGroup = 16;           // replicates whose accumulators a wave holds at once (4 Philox calls)

// Poisson(1) count of a uniform 32-bit word: #{ j : u >= T_j }, T_j = rne(2^32 sum_{i<=j} e^-1 / i!)
TWOSD_HD int boot_count_of_word(uint32_t u) {
    return (int)(u >= 0x5e2d58d9u) + (int)(u >= 0xbc5ab1b1u) + (int)(u >= 0xeb715e1eu) + (int)(u >= 0xfb239797u) +
           (int)(u >= 0xff1025f6u) + (int)(u >= 0xffd90f3cu) + (int)(u >= 0xfffa8b72u) + (int)(u >= 0xffff540cu) +
           (int)(u >= 0xffffed1fu) + (int)(u >= 0xfffffe21u) + (int)(u >= 0xffffffd5u) + (int)(u >= 0xfffffffcu);
}

// the four counts of replicates 4 Q .. 4 Q + 3 for global scenario g
TWOSD_HD Philox4 boot_words(unsigned long long g, int Q, unsigned long long seed) {
    return philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)Q, 1u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// GR (here and below): the draw's index is the scenario's group, first / off count groups and G is
// the group size (a variance-reduced stream: every member of a group carries its group's count);
// !GR: the scenario itself, G unused.  A 32-bit division per lane: a call's scenarios stay below 2^31.
template <bool GR>
__device__ __forceinline__ unsigned long long boot_index(unsigned long long off, int s, unsigned G) {
    if constexpr (GR) return off + (unsigned long long)((unsigned)s / G);
    else return off + (unsigned long long)s;
}

template <bool GR>
__global__ void __launch_bounds__(256) boot_counts_kernel(int M, unsigned long long seed, unsigned long long first, long long count,
                                                          uint8_t *__restrict__ out, unsigned G) {
    const int nq = (M + 3) / 4;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= count * nq) return;
    const long long s = idx / nq;
    const int Q = (int)(idx - s * nq);
    Philox4 r;
    if constexpr (GR) r = boot_words(boot_index<true>(first, (int)s, G), Q, seed);   // s < count <= 2^24
    else r = boot_words(first + (unsigned long long)s, Q, seed);
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (4 * Q + t < M) out[s * M + 4 * Q + t] = (uint8_t)boot_count_of_word(r.v[t]);
}

// out[0] += sum q_s, out[1 + b] += sum c_b(s) q_s over s < n; blockIdx.y = the Philox call Q of four
// replicates, the last y the identity row.  Integer sums: any order gives the same bits.  One atomic
// per block and replicate (a few blocks: every wave adding to the same 33 words took 0.5 ms).
// LIST (here and below): the walk is over the n entries of a tail handle's list (scen[i] ascending
// scenario indices, picks[i] by list position), entry i with the weight and the count of scenario
// scen[i] -- never of the list position: the row of a pick handle with -1 outside the list.  !LIST:
// the scenarios 0 .. n - 1, scen unused.
template <bool GR, bool LIST>
__global__ void __launch_bounds__(256) boot_weight_kernel(int n, const double *__restrict__ w, double scale, int M,
                                                          unsigned long long seed, unsigned long long off,
                                                          unsigned long long *__restrict__ out, unsigned G,
                                                          const int *__restrict__ scen) {
    __shared__ unsigned long long sh[4][4];
    const int nq = (M + 3) / 4, Q = blockIdx.y;
    unsigned long long a[4] = {0ull, 0ull, 0ull, 0ull};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        int s = i;
        if constexpr (LIST) s = scen[i];
        const unsigned long long q = reform_q(w[s], scale);
        if (Q == nq) { a[0] += q; continue; }
        const Philox4 r = boot_words(boot_index<GR>(off, s, G), Q, seed);
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] += (unsigned long long)boot_count_of_word(r.v[t]) * q;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
        for (int o = 32; o > 0; o >>= 1) a[t] += __shfl_xor(a[t], o);
    if ((threadIdx.x & 63) == 0)
        for (int t = 0; t < 4; ++t) sh[threadIdx.x >> 6][t] = a[t];
    __syncthreads();
    if (threadIdx.x >= 4) return;
    const int t = threadIdx.x;
    const unsigned long long v = sh[0][t] + sh[1][t] + sh[2][t] + sh[3][t];
    if (!v) return;
    if (Q == nq) {
        if (t == 0) atomicAdd(&out[0], v);
    } else if (4 * Q + t < M) {
        atomicAdd(&out[1 + 4 * Q + t], v);
    }
}

// hist[row][v] += sum over the scenarios s < n with pick v of c_row(s) q_s, through a block
// histogram in LDS: blockIdx.y = the Philox call Q of four replicates (the last y: the identity
// row), blockIdx.z = a window of kBootVW vertices (a pick outside it is another block's).  Integer
// sums: the atomics' order does not show in the result.
constexpr int kBootVW = 2048;
template <bool GR, bool LIST>
__global__ void __launch_bounds__(1024) boot_hist_kernel(int n, int nv, int nvs, int M, const int *__restrict__ picks,
                                                         const double *__restrict__ w, double scale, unsigned long long seed,
                                                         unsigned long long off, unsigned long long *__restrict__ hist, unsigned G,
                                                         const int *__restrict__ scen) {
    __shared__ unsigned long long hl[4 * kBootVW];
    const int nq = (M + 3) / 4, Q = blockIdx.y;
    const int v0 = blockIdx.z * kBootVW, v1 = min(nv, v0 + kBootVW);
    for (int i = threadIdx.x; i < 4 * kBootVW; i += 1024) hl[i] = 0ull;
    __syncthreads();
    for (int i = blockIdx.x * 1024 + threadIdx.x; i < n; i += gridDim.x * 1024) {
        const int pick = picks[i];
        if (pick < v0 || pick >= v1) continue;
        int s = i;
        if constexpr (LIST) s = scen[i];
        const unsigned long long q = reform_q(w[s], scale);
        if (!q) continue;
        if (Q == nq) {
            __hip_atomic_fetch_add(&hl[pick - v0], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            continue;
        }
        const Philox4 r = boot_words(boot_index<GR>(off, s, G), Q, seed);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int cnt = (4 * Q + t < M) ? boot_count_of_word(r.v[t]) : 0;
            if (cnt)
                __hip_atomic_fetch_add(&hl[t * kBootVW + pick - v0], (unsigned long long)cnt * q, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * kBootVW; i += 1024) {
        const unsigned long long h = hl[i];
        if (!h) continue;
        const int row = Q == nq ? 0 : 1 + 4 * Q + i / kBootVW;
        atomicAdd(&hist[(size_t)row * nvs + v0 + i % kBootVW], h);
    }
}

struct BootParams {
    int n, k, k4, nv, M, ngroups, tpb;   // tpb: 64-scenario tiles per block
    int G;                               // sampling group (grouped kernels; off then counts groups)
    double scale;
    unsigned long long seed, off;
    const double *dv, *w, *PK;
    const int *picks;
    double *slots;                       // nchunks x (M + 1) x k
    const int *scen;                     // LIST: n is the list's length, picks go by list position
};

// KE: elements per lane (k <= 64 KE).  GM: whose count a scenario carries --
//   0  its own (the i.i.d. epigraph)
//   1  its group's, any G: groups straddle tiles, waves and chunks, and a count is a pure function of
//      the group index, so each lane draws the words of its own scenario's group
//   2  its group's, G a multiple of 64: off and every tile start are multiples of 64, so a tile lies
//      inside one group and its 16 counts are wave-uniform -- one draw per tile, held in SGPRs, and
//      the tile's terms are summed once and weighed by the 16 counts at the tile's end
// LIST: the tiles are 64 entries of a tail handle's list, each lane draws the words of its own entry's
// scenario (or of that scenario's group) and only the rows dv[scen_i] are read; the shards are
// reform_shards(nt) over the list.  A tile of the list straddles groups whatever G is: no GM == 2.
template <int KE, int GM, bool LIST>
__global__ void __launch_bounds__(256) boot_reform_kernel(BootParams P) {
    static_assert(!(LIST && GM == 2), "a tile of a tail handle's list never lies inside one group");
    __shared__ double comb[(kBootGroup + 1) * KE * 64];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = blockIdx.x % P.ngroups, chunk = blockIdx.x / P.ngroups;
    const int ntiles = (P.n + 63) >> 6;
    const int t0 = chunk * P.tpb, t1 = min(ntiles, t0 + P.tpb);
    int ec[KE];                       // this lane's elements, clamped to k - 1
#pragma unroll
    for (int u = 0; u < KE; ++u) ec[u] = min(lane + 64 * u, P.k - 1);
    double acc[kBootGroup + 1][KE];
#pragma unroll
    for (int r = 0; r <= kBootGroup; ++r)
#pragma unroll
        for (int u = 0; u < KE; ++u) acc[r][u] = 0.0;

    for (int t = t0 + wid; t < t1; t += 4) {
        // lanes = the tile's scenarios (LIST: its list entries)
        const int li = t * 64 + lane;
        const bool valid = li < P.n;
        int s = li;
        if constexpr (LIST) s = valid ? P.scen[li] : 0;
        const int pick = valid ? P.picks[li] : -1;
        const bool ok = pick >= 0 && pick < P.nv;          // a scenario without a pick weighs in W only
        const unsigned long long q = ok ? reform_q(P.w[s], P.scale) : 0ull;
        unsigned chi[kBootGroup];                           // high word of (double)count: 0 for count 0
#pragma unroll
        for (int qd = 0; qd < kBootGroup / 4; ++qd) {
            const int Q = grp * (kBootGroup / 4) + qd;
            Philox4 r;
            r.v[0] = r.v[1] = r.v[2] = r.v[3] = 0u;
            if (4 * Q < P.M) r = boot_words(boot_index<GM != 0>(P.off, GM == 2 ? t * 64 : s, (unsigned)P.G), Q, P.seed);   // wave-uniform
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const int cnt = (4 * Q + tt < P.M) ? boot_count_of_word(r.v[tt]) : 0;
                chi[4 * qd + tt] = (unsigned)__double2hiint((double)cnt);
                if constexpr (GM == 2) chi[4 * qd + tt] = (unsigned)__builtin_amdgcn_readfirstlane((int)chi[4 * qd + tt]);
            }
        }
        // GM == 2: the identity row's accumulator takes the tile's terms alone, from 0
        double idsum[KE];
        if constexpr (GM == 2) {
#pragma unroll
            for (int u = 0; u < KE; ++u) { idsum[u] = acc[kBootGroup][u]; acc[kBootGroup][u] = 0.0; }
        }
        const double qf = (double)q;
        const int qlo = __double2loint(qf), qhi = __double2hiint(qf);
        const int pk0 = ok ? pick : 0;
        // lanes = elements; the scenarios go by four at a time, the next four's rows (8 KE loads of
        // 512 B each) in flight under the current four's arithmetic.  A lane past k reads element
        // k - 1 again (no divergent load) and its sums are never stored; a step past the tile's
        // last scenario reads that scenario again with weight 0.
        const int nvalid = min(64, P.n - t * 64);
        const double *dvt = P.dv + (size_t)(t * 64) * P.k;
        auto load4 = [&](int i0, double (&d)[4][KE], double (&p)[4][KE]) {
#pragma unroll
            for (int u4 = 0; u4 < 4; ++u4) {
                const int i = min(i0 + u4, nvalid - 1);
                const int pv = __builtin_amdgcn_readlane(pk0, i);
                const double *row = dvt + (size_t)i * P.k;
                if constexpr (LIST) row = P.dv + (size_t)__builtin_amdgcn_readlane(s, i) * P.k;
#pragma unroll
                for (int u = 0; u < KE; ++u) {
                    d[u4][u] = row[ec[u]];
                    p[u4][u] = P.PK[(size_t)pv * P.k4 + ec[u]];
                }
            }
        };
        auto work4 = [&](int i0, const double (&d)[4][KE], const double (&p)[4][KE]) {
#pragma unroll
            for (int u4 = 0; u4 < 4; ++u4) {
                const int i = min(i0 + u4, 63);
                const double wq = i0 + u4 < nvalid ? __hiloint2double(__builtin_amdgcn_readlane(qhi, i), __builtin_amdgcn_readlane(qlo, i)) : 0.0;
                double term[KE];
#pragma unroll
                for (int u = 0; u < KE; ++u) term[u] = wq * p[u4][u] * d[u4][u];
#pragma unroll
                for (int r = 0; r < (GM == 2 ? 0 : kBootGroup); ++r) {   // GM == 2: at the tile's end
                    const double cd = __hiloint2double(__builtin_amdgcn_readlane((int)chi[r], i), 0);   // wave-uniform count
#pragma unroll
                    for (int u = 0; u < KE; ++u) acc[r][u] = fma(cd, term[u], acc[r][u]);
                }
#pragma unroll
                for (int u = 0; u < KE; ++u) acc[kBootGroup][u] += term[u];
            }
        };
        double da[4][KE], pa[4][KE], db[4][KE], pb[4][KE];
        load4(0, da, pa);
        for (int i0 = 0; i0 < nvalid; i0 += 8) {
            if (i0 + 4 < nvalid) load4(i0 + 4, db, pb);
            work4(i0, da, pa);
            if (i0 + 4 >= nvalid) break;
            if (i0 + 8 < nvalid) load4(i0 + 8, da, pa);
            work4(i0 + 4, db, pb);
        }
        if constexpr (GM == 2) {   // the tile's sum weighed by its 16 counts (SGPR pairs), then back into the identity row
#pragma unroll
            for (int u = 0; u < KE; ++u) {
                const double tsum = acc[kBootGroup][u];
#pragma unroll
                for (int r = 0; r < kBootGroup; ++r) acc[r][u] = fma(__hiloint2double((int)chi[r], 0), tsum, acc[r][u]);
                acc[kBootGroup][u] = idsum[u] + tsum;
            }
        }
    }
    // the block's four waves combined in wave order
    for (int wv = 0; wv < 4; ++wv) {
        if (wid == wv) {
#pragma unroll
            for (int r = 0; r <= kBootGroup; ++r)
#pragma unroll
                for (int u = 0; u < KE; ++u) {
                    double &d = comb[(r * KE + u) * 64 + lane];
                    d = wv == 0 ? acc[r][u] : d + acc[r][u];
                }
        }
        __syncthreads();
    }
    const int B = P.M + 1;
    double *out = P.slots + (size_t)chunk * B * P.k;
    for (int idx = threadIdx.x; idx < (kBootGroup + 1) * KE * 64; idx += 256) {
        const int r = idx / (KE * 64), e = idx % (KE * 64);
        const int row = r == kBootGroup ? (grp == 0 ? 0 : -1) : 1 + grp * kBootGroup + r;
        if (row >= 0 && row < B && e < P.k) out[(size_t)row * P.k + e] = comb[idx];
    }
}

static PickSet *pick_of(twosd_ctx *c, int handle) {
    if (handle < 0 || handle >= (int)c->reform.picks.size() || !c->reform.picks[handle].live) return nullptr;
    return &c->reform.picks[handle];
}

// the first slot of the handle table that is not live (a new one at its end): the caller fills it
PickSet *pick_slot(twosd_ctx *c, int *id) {
    std::vector<PickSet> &v = c->reform.picks;
    int i = 0;
    while (i < (int)v.size() && v[i].live) ++i;
    if (i == (int)v.size()) v.emplace_back();
    *id = i;
    return &v[i];
}

// a usable handle, or the error code with its message
int usable_pick(twosd_ctx *c, int handle, const char *what, PickSet **out) {
    PickSet *h = pick_of(c, handle);
    if (!h)
        return fail(TWOSD_E_ARG, "%s: pick handle %d does not exist (released, or dropped by twosd_set_template / "
                    "twosd_set_random_positions)", what, handle);
    if (h->stale || h->nv > c->dvs.size)
        return fail(TWOSD_E_STATE, "%s: pick handle %d names vertices below %d, but the vertex set was cleared or truncated "
                    "below that since", what, handle, h->nv);
    *out = h;
    return TWOSD_OK;
}

static int boot_layout(twosd_ctx *c, int epi, int H, const int *handles, int M, const char *what, BootLayout *L) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "%s: no template", what);
    if (H < 1 || !handles) return fail(TWOSD_E_ARG, "%s: H = %d handles (at least 1)", what, H);
    if (M < 0 || M > kBootMaxM) return fail(TWOSD_E_ARG, "%s: M = %d replicates outside [0, %d]", what, M, kBootMaxM);
    if (c->k > 127) return fail(TWOSD_E_UNSUPPORTED, "k = %d random elements exceeds the cut kernel envelope (127)", c->k);
    int nvs = 1;
    for (int j = 0; j < H; ++j) {
        PickSet *h = nullptr;
        int rc = usable_pick(c, handles[j], what, &h);
        if (rc) return rc;
        if (epi >= 0 && h->epi != epi)
            return fail(TWOSD_E_ARG, "%s: pick handle %d belongs to epigraph %d, not %d", what, handles[j], h->epi, epi);
        nvs = std::max(nvs, h->nv);
    }
    *L = boot_offsets(H, M, nvs, c->k);
    return TWOSD_OK;
}

// Kernel selection, one function per family.  G == 1 draws by the scenario, G > 1 by its group;
// list: the walk is over a tail handle's list.
using BootWeightFn = decltype(&boot_weight_kernel<false, false>);
static BootWeightFn boot_weight_fn(int G, bool list) {
    return G == 1 ? (list ? boot_weight_kernel<false, true> : boot_weight_kernel<false, false>)
                  : (list ? boot_weight_kernel<true, true> : boot_weight_kernel<true, false>);
}

using BootHistFn = decltype(&boot_hist_kernel<false, false>);
static BootHistFn boot_hist_fn(int G, bool list) {
    return G == 1 ? (list ? boot_hist_kernel<false, true> : boot_hist_kernel<false, false>)
                  : (list ? boot_hist_kernel<true, true> : boot_hist_kernel<true, false>);
}

// GM = 0 for G == 1; 2 where a tile lies inside one group (G a multiple of 64, never on a list); else 1
using BootReformFn = void (*)(BootParams);
template <int KE>
static BootReformFn boot_reform_fn(int G, bool list) {
    if (G == 1) return list ? boot_reform_kernel<KE, 0, true> : boot_reform_kernel<KE, 0, false>;
    if (G % 64 == 0 && !list) return boot_reform_kernel<KE, 2, false>;
    return list ? boot_reform_kernel<KE, 1, true> : boot_reform_kernel<KE, 1, false>;
}

static BootReformFn boot_reform_fn(int k, int G, bool list) {   // k <= 64: one element per lane
    return k <= 64 ? boot_reform_fn<1>(G, list) : boot_reform_fn<2>(G, list);
}

// G > 1: the counts of a variance-reduced stream's groups (off and every scenario count are whole
// groups: the callers check); the kernels then index their draws by off / G + s / G
static int boot_partial_impl(twosd_ctx *c, int epi, const BootLayout &L, const int *handles, int M, unsigned long long seed,
                             unsigned long long off, int G, double total_weight, unsigned long long *d_u64, double *d_f64) {
    const EpiDevice &E = c->epis[epi];
    const int k = c->k, B = L.B;
    const double scale = kReformFix / total_weight;
    const double *PK = nullptr;
    int k4 = 0, rc;
    if ((rc = cut_pk_current(c, &PK, &k4))) return rc;
    HIPCHK(hipMemsetAsync(d_u64, 0, sizeof(unsigned long long) * L.n_u64, c->stream));
    const int nq = (M + 3) / 4;
    if (G > 1) off /= (unsigned long long)G;   // the one 64-bit division of a grouped call
    // scen: a tail handle's list (the LIST kernels walk its n entries), nullptr for the scenarios 0 .. n - 1
    auto weights = [&](int n, const int *scen, unsigned long long *out) {
        const dim3 grid(std::max(1, std::min((n + 8191) / 8192, 32)), nq + 1);
        hipLaunchKernelGGL(boot_weight_fn(G, scen != nullptr), grid, dim3(256), 0, c->stream, n, E.d_w.p, scale, M, seed, off, out,
                           (unsigned)G, scen);
    };
    if (E.count > 0) weights(E.count, nullptr, d_u64);
    const int ngroups = std::max(1, (M + kBootGroup - 1) / kBootGroup);
    size_t slots_need = 1;
    for (int j = 0; j < L.H; ++j) {
        const PickSet &h = c->reform.picks[handles[j]];
        if (h.n > E.count)
            return fail(TWOSD_E_STATE, "reform: pick handle %d holds %d scenarios, epigraph %d only %d", handles[j], h.n, epi, E.count);
        if (h.entries() > 0)   // a pick handle's n >= 1 (picks_keep); an empty tail launches nothing
            slots_need = std::max(slots_need, (size_t)reform_shards(h.entries()).nchunks * B * k);
    }
    if ((rc = c->reform.slots.fit(slots_need))) return rc;   // once, before the first launch that writes it
    for (int j = 0; j < L.H; ++j) {
        // the handle's words of the layout: W_j, the histogram rows and S, over its scenarios or over
        // its tail's compact list (nothing outside the tail is read)
        const PickSet &h = c->reform.picks[handles[j]];
        const int entries = h.entries();
        const int *scen = h.is_tail() ? h.scen.p : nullptr;
        double *Sj = d_f64 + (size_t)j * B * k;
        if (entries == 0) {   // no launch over an empty list: W and the histogram rows stay 0, S is set to 0 -- the zero cut
            if (k > 0) HIPCHK(hipMemsetAsync(Sj, 0, sizeof(double) * (size_t)B * k, c->stream));
            continue;
        }
        weights(entries, scen, d_u64 + L.o_wj + (size_t)j * B);
        const dim3 hgrid(std::max(1, std::min((entries + 8191) / 8192, 64)), nq + 1, (h.nv + kBootVW - 1) / kBootVW);
        hipLaunchKernelGGL(boot_hist_fn(G, scen != nullptr), hgrid, dim3(1024), 0, c->stream, entries, h.nv, L.nvs, M, h.d.p, E.d_w.p,
                           scale, seed, off, d_u64 + L.o_hist + (size_t)j * B * L.nvs, (unsigned)G, scen);
        if (k == 0) continue;
        const ReformShards sh = reform_shards(entries);
        BootParams P{};
        P.n = entries; P.k = k; P.k4 = k4; P.nv = h.nv; P.M = M; P.ngroups = ngroups; P.tpb = sh.tpb; P.G = G;
        P.scale = scale; P.seed = seed; P.off = off;
        P.dv = E.d_dv; P.w = E.d_w; P.PK = PK; P.picks = h.d; P.scen = scen;
        P.slots = c->reform.slots;
        hipLaunchKernelGGL(boot_reform_fn(k, G, scen != nullptr), dim3(sh.nchunks * ngroups), dim3(256), 0, c->stream, P);
        reform_sum_shards(c, true, sh.nchunks, B * k, c->reform.slots.p, Sj);
    }
    HIPCHK(hipGetLastError());
    return TWOSD_OK;
}

static int boot_finalize_impl(twosd_ctx *c, const BootLayout &L, const int *handles, double total_weight,
                              const unsigned long long *d_u64, const double *d_f64, double *alpha, double *beta,
                              double *weight_mark, double *total_out) {
    ReformState &S = c->reform;
    const int B = L.B, H = L.H, n1 = c->n1, k = c->k;
    int rc;
    if ((rc = reform_prepare(c, B, H, L.nvs))) return rc;
    const size_t rows = (size_t)B * H;
    const double wunit = total_weight / kReformFix;
    for (int j = 0; j < H; ++j) {
        const PickSet &h = S.picks[handles[j]];
        if ((rc = reform_finalize_block(c, B, H, j, h.nv, L.nvs, d_u64 + L.o_hist + (size_t)j * B * L.nvs, d_f64 + (size_t)j * B * k,
                                        d_u64 + L.o_wj + (size_t)j * B, wunit)))
            return rc;
    }
    std::vector<unsigned long long> tw(B);
    HIPCHK(hipMemcpyAsync(alpha, S.d_alpha, sizeof(double) * rows, hipMemcpyDeviceToHost, c->stream));
    if (n1 > 0) HIPCHK(hipMemcpyAsync(beta, S.d_beta, sizeof(double) * rows * n1, hipMemcpyDeviceToHost, c->stream));
    if (weight_mark) HIPCHK(hipMemcpyAsync(weight_mark, S.d_wm, sizeof(double) * rows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(tw.data(), d_u64, sizeof(unsigned long long) * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (total_out)
        for (int b = 0; b < B; ++b) total_out[b] = (double)tw[b] * wunit;
    return TWOSD_OK;
}

}  // namespace twosd

using namespace twosd;

extern "C" int twosd_bootstrap_count_of_word(uint32_t u) { return boot_count_of_word(u); }

// G > 1: scenario first_index + s carries the counts of group (first_index + s) / G (whole groups: the caller checks)
static int bootstrap_counts_impl(twosd_ctx *c, int M, uint64_t seed, uint64_t first_index, int64_t count, int G, uint8_t *out) {
    if (!c) return fail(TWOSD_E_ARG, "bootstrap_counts: ctx is NULL");
    if (M < 1 || M > kBootMaxM) return fail(TWOSD_E_ARG, "bootstrap_counts: M = %d replicates outside [1, %d]", M, kBootMaxM);
    if (count < 0 || count > (1ll << 24) || (count > 0 && !out))
        return fail(TWOSD_E_ARG, "bootstrap_counts: count = %lld outside [0, 2^24] or out NULL", (long long)count);
    if (count == 0) return TWOSD_OK;
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = c->reform.counts.fit((size_t)count * M))) return rc;
    const long long total = count * ((M + 3) / 4);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (G == 1)
        hipLaunchKernelGGL(boot_counts_kernel<false>, grid, dim3(256), 0, c->stream, M, (unsigned long long)seed,
                           (unsigned long long)first_index, (long long)count, c->reform.counts.p, 1u);
    else
        hipLaunchKernelGGL(boot_counts_kernel<true>, grid, dim3(256), 0, c->stream, M, (unsigned long long)seed,
                           (unsigned long long)first_index / (unsigned long long)G, (long long)count, c->reform.counts.p, (unsigned)G);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, c->reform.counts, (size_t)count * M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return TWOSD_OK;
}

extern "C" int twosd_bootstrap_counts(twosd_ctx *c, int M, uint64_t seed, uint64_t first_index, int64_t count, uint8_t *out) {
    return bootstrap_counts_impl(c, M, seed, first_index, count, 1, out);
}

extern "C" int twosd_bootstrap_counts_vr(twosd_ctx *c, int M, uint64_t seed, uint64_t first_index, int64_t count, uint8_t *out,
                                         const twosd_sampling *plan) {
    int mode, G, rc;
    if ((rc = sampling_plan(plan, "bootstrap_counts", &mode, &G))) return rc;
    if (G == 1) return twosd_bootstrap_counts(c, M, seed, first_index, count, out);
    if ((rc = whole_groups("bootstrap_counts", "first_index", first_index, G)) ||
        (count > 0 && (rc = whole_groups("bootstrap_counts", "count", (unsigned long long)count, G))))
        return rc;
    return bootstrap_counts_impl(c, M, seed, first_index, count, G, out);
}

extern "C" int twosd_picks_keep(twosd_ctx *c, int epi, int *handle) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "picks_keep: no template");
    if (!handle) return fail(TWOSD_E_ARG, "picks_keep: handle is NULL");
    int rc = cut_last_usable(c, epi, "picks_keep", "keep");
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    int id = 0;
    PickSet &h = *pick_slot(c, &id);
    if ((rc = h.d.alloc(c->last_cut_n))) return rc;
    HIPCHK(hipMemcpyAsync(h.d, cut_last_arg(c), sizeof(int) * c->last_cut_n, hipMemcpyDeviceToDevice, c->stream));
    h.epi = epi; h.n = c->last_cut_n; h.nv = c->last_cut_nv; h.live = true; h.stale = false;
    *handle = id;
    return TWOSD_OK;
}

extern "C" int twosd_picks_info(twosd_ctx *c, int handle, int *epi, int *n, int *nv) {
    if (!c) return fail(TWOSD_E_ARG, "picks_info: ctx is NULL");
    PickSet *h = nullptr;
    int rc = usable_pick(c, handle, "picks_info", &h);
    if (rc) return rc;
    if (epi) *epi = h->epi;
    if (n) *n = h->n;
    if (nv) *nv = h->nv;
    return TWOSD_OK;
}

extern "C" int twosd_picks_get(twosd_ctx *c, int handle, int *out) {
    if (!c || !out) return fail(TWOSD_E_ARG, "picks_get: NULL");
    PickSet *h = nullptr;
    int rc = usable_pick(c, handle, "picks_get", &h);
    if (rc) return rc;
    if (h->is_tail())
        return fail(TWOSD_E_ARG, "picks_get: handle %d is a tail handle (%d of %d scenarios): read it with twosd_tail_get", handle,
                    h->nt, h->n);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(out, h->d, sizeof(int) * h->n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return TWOSD_OK;
}

extern "C" int twosd_picks_release(twosd_ctx *c, int handle) {
    if (!c) return fail(TWOSD_E_ARG, "picks_release: ctx is NULL");
    PickSet *h = pick_of(c, handle);
    if (!h) return fail(TWOSD_E_ARG, "picks_release: pick handle %d does not exist", handle);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));   // a re-formation reading it has finished
    *h = PickSet();
    return TWOSD_OK;
}

extern "C" int twosd_picks_count(twosd_ctx *c, int *live) {
    if (!c || !live) return fail(TWOSD_E_ARG, "picks_count: NULL");
    int n = 0;
    for (const PickSet &h : c->reform.picks) n += h.live ? 1 : 0;
    *live = n;
    return TWOSD_OK;
}

extern "C" int twosd_reform_partial_len(twosd_ctx *c, int H, const int *handles, int M, int64_t *n_u64, int64_t *n_f64) {
    BootLayout L;
    int rc = boot_layout(c, -1, H, handles, M, "reform_partial_len", &L);
    if (rc) return rc;
    if (n_u64) *n_u64 = (int64_t)L.n_u64;
    if (n_f64) *n_f64 = (int64_t)L.n_f64;
    return TWOSD_OK;
}

static int check_epi(twosd_ctx *c, int epi, const char *what) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "%s: no template", what);
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "%s: epigraph %d does not exist", what, epi);
    return TWOSD_OK;
}

// under a plan with group G the observations are the groups: index_offset, the epigraph's scenario
// count and every handle's N_j must be whole groups
static int reform_whole_groups(twosd_ctx *c, int epi, int H, const int *handles, uint64_t index_offset, int G, const char *what) {
    if (G == 1) return TWOSD_OK;
    int rc;
    if ((rc = whole_groups(what, "index_offset", index_offset, G))) return rc;
    if (c->epis[epi].count % G)
        return fail(TWOSD_E_ARG, "%s: epigraph %d holds %d scenarios, no multiple of the sampling group %d", what, epi,
                    c->epis[epi].count, G);
    for (int j = 0; j < H; ++j) {
        const PickSet &h = c->reform.picks[handles[j]];
        if (h.n % G)
            return fail(TWOSD_E_ARG, "%s: pick handle %d holds %d scenarios, no multiple of the sampling group %d", what, handles[j],
                        h.n, G);
    }
    return TWOSD_OK;
}

static int reform_partial_impl(twosd_ctx *c, int epi, int H, const int *handles, int M, uint64_t seed, uint64_t index_offset, int G,
                               double total_weight, uint64_t *d_u64, double *d_f64) {
    BootLayout L;
    int rc = boot_layout(c, -1, H, handles, M, "reform_partial", &L);   // a dropped handle is named before the epigraph
    if (rc || (rc = check_epi(c, epi, "reform_partial")) || (rc = boot_layout(c, epi, H, handles, M, "reform_partial", &L))) return rc;
    if (!d_u64 || !d_f64) return fail(TWOSD_E_ARG, "reform_partial: device buffers NULL");
    if (!(total_weight > 0.0) || !std::isfinite(total_weight)) return fail(TWOSD_E_ARG, "reform_partial: total_weight must be > 0");
    if ((rc = reform_whole_groups(c, epi, H, handles, index_offset, G, "reform_partial"))) return rc;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = boot_partial_impl(c, epi, L, handles, M, seed, index_offset, G, total_weight, (unsigned long long *)d_u64, d_f64)))
        return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return TWOSD_OK;
}

extern "C" int twosd_reform_partial(twosd_ctx *c, int epi, int H, const int *handles, int M, uint64_t seed, uint64_t index_offset,
                                    double total_weight, uint64_t *d_u64, double *d_f64) {
    return reform_partial_impl(c, epi, H, handles, M, seed, index_offset, 1, total_weight, d_u64, d_f64);
}

extern "C" int twosd_reform_partial_vr(twosd_ctx *c, int epi, int H, const int *handles, int M, uint64_t seed, uint64_t index_offset,
                                       double total_weight, uint64_t *d_u64, double *d_f64, const twosd_sampling *plan) {
    int mode, G, rc;
    if ((rc = sampling_plan(plan, "reform_partial", &mode, &G))) return rc;
    if (G == 1) return twosd_reform_partial(c, epi, H, handles, M, seed, index_offset, total_weight, d_u64, d_f64);
    return reform_partial_impl(c, epi, H, handles, M, seed, index_offset, G, total_weight, d_u64, d_f64);
}

extern "C" int twosd_reform_finalize(twosd_ctx *c, int H, const int *handles, int M, double total_weight, const uint64_t *d_u64,
                                     const double *d_f64, double *alpha, double *beta, double *weight_mark, double *total_weight_out) {
    BootLayout L;
    int rc = boot_layout(c, -1, H, handles, M, "reform_finalize", &L);
    if (rc) return rc;
    if (!d_u64 || !d_f64 || !alpha || (c->n1 > 0 && !beta)) return fail(TWOSD_E_ARG, "reform_finalize: NULL buffers");
    if (!(total_weight > 0.0) || !std::isfinite(total_weight)) return fail(TWOSD_E_ARG, "reform_finalize: total_weight must be > 0");
    HIPCHK(hipSetDevice(c->device));
    return boot_finalize_impl(c, L, handles, total_weight, (const unsigned long long *)d_u64, d_f64, alpha, beta, weight_mark,
                              total_weight_out);
}

static int reform_cuts_impl(twosd_ctx *c, int epi, int H, const int *handles, int M, uint64_t seed, uint64_t index_offset, int G,
                            double *alpha, double *beta, double *weight_mark, double *total_weight) {
    BootLayout L;
    int rc = boot_layout(c, -1, H, handles, M, "reform_cuts", &L);
    if (rc || (rc = check_epi(c, epi, "reform_cuts")) || (rc = boot_layout(c, epi, H, handles, M, "reform_cuts", &L))) return rc;
    if (!alpha || (c->n1 > 0 && !beta)) return fail(TWOSD_E_ARG, "reform_cuts: alpha/beta NULL");
    const EpiDevice &E = c->epis[epi];
    if (!(E.total_weight > 0.0)) return fail(TWOSD_E_STATE, "reform_cuts: epigraph %d holds no scenario weight", epi);
    if ((rc = reform_whole_groups(c, epi, H, handles, index_offset, G, "reform_cuts"))) return rc;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = c->reform.u64.fit(L.n_u64)) || (rc = c->reform.f64.fit(L.n_f64))) return rc;
    HIPCHK(hipEventRecord(c->ev[EV_MARK_0], c->stream));
    if ((rc = boot_partial_impl(c, epi, L, handles, M, seed, index_offset, G, E.total_weight, c->reform.u64, c->reform.f64))) return rc;
    HIPCHK(hipEventRecord(c->ev[EV_MARK_1], c->stream));
    if ((rc = boot_finalize_impl(c, L, handles, E.total_weight, c->reform.u64, c->reform.f64, alpha, beta, weight_mark, total_weight)))
        return rc;
    HIPCHK(hipEventRecord(c->ev[EV_MARK_2], c->stream));
    HIPCHK(hipEventSynchronize(c->ev[EV_MARK_2]));
    float ms1 = 0, ms2 = 0;
    hipEventElapsedTime(&ms1, c->ev[EV_MARK_0], c->ev[EV_MARK_1]);
    hipEventElapsedTime(&ms2, c->ev[EV_MARK_1], c->ev[EV_MARK_2]);
    c->reform.ms[0] = ms1;
    c->reform.ms[1] = ms2;
    return TWOSD_OK;
}

extern "C" int twosd_reform_cuts(twosd_ctx *c, int epi, int H, const int *handles, int M, uint64_t seed, uint64_t index_offset,
                                 double *alpha, double *beta, double *weight_mark, double *total_weight) {
    return reform_cuts_impl(c, epi, H, handles, M, seed, index_offset, 1, alpha, beta, weight_mark, total_weight);
}

extern "C" int twosd_reform_cuts_vr(twosd_ctx *c, int epi, int H, const int *handles, int M, uint64_t seed, uint64_t index_offset,
                                    double *alpha, double *beta, double *weight_mark, double *total_weight,
                                    const twosd_sampling *plan) {
    int mode, G, rc;
    if ((rc = sampling_plan(plan, "reform_cuts", &mode, &G))) return rc;
    if (G == 1) return twosd_reform_cuts(c, epi, H, handles, M, seed, index_offset, alpha, beta, weight_mark, total_weight);
    return reform_cuts_impl(c, epi, H, handles, M, seed, index_offset, G, alpha, beta, weight_mark, total_weight);
}

extern "C" int twosd_reform_last_ms(twosd_ctx *c, double *ms2) {
    if (!c || !ms2) return fail(TWOSD_E_ARG, "reform_last_ms: NULL");
    ms2[0] = c->reform.ms[0];
    ms2[1] = c->reform.ms[1];
    return TWOSD_OK;
}
