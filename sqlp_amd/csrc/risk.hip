// risk.hip -- mean-CVaR recourse on the device: the weighted quantile selection (VaR, CVaR and the
// tail weight of a set of values) and the tail cut, a cut re-formed from the last cut's picks
// with the scenarios at or below eta weighed 0.
//
// Reference: none (yhz0/SQLP optimises the expectation only).  Rockafellar and Uryasev:
//     CVaR_a(h) = min_eta  eta + E[(h - eta)+] / (1 - a),  attained at eta = VaR_a(h).
//
// Selection.  An entry counts when its status is optimal (or status is NULL); its integer weight is
// q_s = rn(w_s scale) (reform.h's weight, scale 2^58 / total weight), or 1 without weights.  With
// Q = sum q_s and t = ceil(level Q) (exact: risk_keys.h, on the host, once per call),
//     VaR = the smallest counted value v with sum_{value <= v} q_s >= t
// found by a most-significant-digit radix select over the order-preserving keys of risk_keys.h:
// 8 passes of 8 bits.  A pass adds the q_s of the entries whose key starts with the prefix found
// so far into a 256-bin uint64 histogram (per block in LDS, flushed with integer atomics: exact
// under any grid and any order), and a one-block kernel picks the digit at which the running sum
// reaches the remaining target, extends the prefix and reduces the target -- the record stays on
// the device between the passes.  After pass 8 the prefix is the key of VaR.
//     tail_q = sum_{value > VaR} q_s,   CVaR = VaR + (sum_{value > VaR} q_s (value_s - VaR)) / ((1 - level) Q)
// The fp64 sum runs over kRiskShards contiguous shards of the index range whatever the grid: a
// block takes shards blockIdx.x, + gridDim.x, ...; per shard every thread sums its stride-256
// entries in index order, the 256 partials go through the fixed LDS tree, and the host adds the
// shards in shard order.  Every product, difference and sum is rounded on its own (no FMA).
//
// Tail cut.  The last cut re-formed from its picks with the weights 1[val_s (+ c0) > eta] q_s:
//   risk_thist_kernel    W_t = sum f_s q_s, the total sum q_s and the per-vertex weights (uint64
//                        block histograms in LDS over windows of 2048 vertices, integer atomics)
//   risk_treform_kernel  one pass over the N x k deltas: a wave walks tiles of 64 scenarios, lanes =
//                        scenarios for pick, weight and flag, then lanes = elements while the tile's
//                        tail scenarios go by (a scenario outside the tail is skipped: its row is
//                        never loaded); the shard layout is reform_layout.h's (a function of N alone)
// then reform.hip's stage, one handle and one row: S_e = the shards' partials in shard order (not the
// bootstrap's eight segments), g, and alpha, beta normalised by W_t (W_t = 0: the zero cut).  The two
// kernels above stay the tail's own (one row, flags from scores, skipped rows), not instantiations of
// boot_kernel.hip's templates: reform.hip's header has the reason and the rule for changing either.
//
// Tail handles (twosd_tail_keep).  The set the tail cut sums over -- the scenarios with
// tail_flag, bit for bit -- as a compact list in the pick handles' table (ReformState::picks), so
// that boot_kernel.hip can re-form the tail row under resampled weights reading the tail's deltas
// only.  Compaction on the device, order-preserving and the same under any grid:
//   risk_tcount_kernel    a wave per 64-scenario tile: one ballot of the flags, the tile's count
//   risk_tscan_kernel     one block: the exclusive scan of the tiles' counts, nt behind the last
//   risk_tscatter_kernel  (scenario, pick) at the tile's offset plus the lane's rank in the ballot
// nt is the one value copied to the host (it sizes the handle's two arrays: 8 bytes per tail scenario).
//
// No floating-point atomics anywhere; TWOSD_RISK_BLOCKS (test knob) sets the grids and must not
// change a bit of any result.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>
#include "reform.h"
#include "risk_keys.h"

namespace twosd {

constexpr int kRiskBits = 8, kRiskBins = 1 << kRiskBits, kRiskPasses = 64 / kRiskBits;
constexpr int kRiskShards = 256;                       // shards of the tail sum (fixed: the result's bits depend on it)
constexpr int kRiskVW = 2048;                          // vertices per LDS histogram window of the tail cut

// the selection record, behind the histograms in RiskState::u64
struct RiskSel {
    unsigned long long prefix, target;   // key digits found so far; what the remaining digits must reach
    unsigned long long total_q, n_bad, n_ok, tail_q;
};
constexpr size_t kRiskHistWords = (size_t)kRiskPasses * kRiskBins;
constexpr size_t kRiskWords = kRiskHistWords + sizeof(RiskSel) / sizeof(unsigned long long);

struct RiskIn {
    long long n;
    const double *val, *w;   // w nullable: unit weights
    const int *st;           // nullable: every entry counts
    double scale, add;       // q = rn(w scale); the value is val + add (one rounded add) when has_add
    int has_add;
};

__device__ __forceinline__ unsigned long long risk_q(const RiskIn &I, long long s) {
    if (!I.w) return 1ull;
    const double w = I.w[s];   // reform_q, written out: through the call the selection kernels take 2 or 3 more VGPRs
    return w > 0.0 ? (unsigned long long)__double2ull_rn(w * I.scale) : 0ull;
}
__device__ __forceinline__ bool risk_counted(const RiskIn &I, long long s) { return !I.st || I.st[s] == TWOSD_LP_OPTIMAL; }
__device__ __forceinline__ double risk_value(const RiskIn &I, long long s) {
    const double v = I.val[s];
    return I.has_add ? __dadd_rn(v, I.add) : v;
}

template <typename T>
__device__ __forceinline__ T risk_block_sum(T v, T *sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// Q, the counted and the left-out entries (integers: any order)
__global__ void __launch_bounds__(256) risk_total_kernel(RiskIn I, RiskSel *__restrict__ sel) {
    __shared__ unsigned long long sh[256];
    unsigned long long q = 0, ok = 0, bad = 0;
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < I.n; s += (long long)gridDim.x * 256) {
        if (!risk_counted(I, s)) { ++bad; continue; }
        ++ok;
        q += risk_q(I, s);
    }
    q = risk_block_sum(q, sh);
    ok = risk_block_sum(ok, sh);
    bad = risk_block_sum(bad, sh);
    if (threadIdx.x == 0) {
        if (q) atomicAdd(&sel->total_q, q);
        if (ok) atomicAdd(&sel->n_ok, ok);
        if (bad) atomicAdd(&sel->n_bad, bad);
    }
}

// pass p: hist[digit p of key] += q over the counted entries whose first p digits are the prefix
__global__ void __launch_bounds__(256) risk_hist_kernel(RiskIn I, int pass, const RiskSel *__restrict__ sel,
                                                        unsigned long long *__restrict__ hist) {
    __shared__ unsigned long long hl[kRiskBins];
    hl[threadIdx.x] = 0ull;   // kRiskBins == blockDim.x
    __syncthreads();
    const unsigned long long prefix = sel->prefix;
    const int shift = 64 - kRiskBits * (pass + 1);
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < I.n; s += (long long)gridDim.x * 256) {
        if (!risk_counted(I, s)) continue;
        const unsigned long long q = risk_q(I, s);
        if (!q) continue;
        const unsigned long long key = risk_key(risk_value(I, s));
        if (pass > 0 && (key >> (shift + kRiskBits)) != prefix) continue;
        __hip_atomic_fetch_add(&hl[(key >> shift) & (kRiskBins - 1)], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    const unsigned long long h = hl[threadIdx.x];
    if (h) atomicAdd(&hist[threadIdx.x], h);
}
static_assert(kRiskBins == 256, "risk_hist_kernel and risk_pick_kernel run one thread per bin");

// one block: the digit d with sum_{j < d} hist[j] < target <= sum_{j <= d} hist[j]
__global__ void __launch_bounds__(256) risk_pick_kernel(const unsigned long long *__restrict__ hist, RiskSel *__restrict__ sel) {
    __shared__ unsigned long long cum[kRiskBins];
    __shared__ unsigned long long target, prefix;
    cum[threadIdx.x] = hist[threadIdx.x];
    if (threadIdx.x == 0) { target = sel->target; prefix = sel->prefix; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int j = 1; j < kRiskBins; ++j) cum[j] += cum[j - 1];
    __syncthreads();
    const unsigned long long lo = threadIdx.x ? cum[threadIdx.x - 1] : 0ull, hi = cum[threadIdx.x];
    if (lo < target && target <= hi) {   // one thread: the bins' sums are non-decreasing
        sel->prefix = (prefix << kRiskBits) | (unsigned long long)threadIdx.x;
        sel->target = target - lo;
    }
}

// tail_q and the shards' sums of q (value - VaR) over the counted entries above VaR (key order)
__global__ void __launch_bounds__(256) risk_tailsum_kernel(RiskIn I, RiskSel *__restrict__ sel, double *__restrict__ part) {
    __shared__ double shd[256];
    __shared__ unsigned long long shq[256];
    const unsigned long long vkey = sel->prefix;
    const double var = risk_unkey(vkey);
    const long long L = (I.n + kRiskShards - 1) / kRiskShards;
    unsigned long long tq = 0;
    for (int b = blockIdx.x; b < kRiskShards; b += gridDim.x) {
        const long long lo = std::min((long long)b * L, I.n), hi = std::min(lo + L, I.n);
        double f = 0.0;
        for (long long s = lo + threadIdx.x; s < hi; s += 256) {
            if (!risk_counted(I, s)) continue;
            const double v = risk_value(I, s);
            if (risk_key(v) <= vkey) continue;
            const unsigned long long q = risk_q(I, s);
            tq += q;
            f = __dadd_rn(f, __dmul_rn((double)q, __dadd_rn(v, -var)));
        }
        f = risk_block_sum(f, shd);
        if (threadIdx.x == 0) part[b] = f;
    }
    tq = risk_block_sum(tq, shq);
    if (threadIdx.x == 0 && tq) atomicAdd(&sel->tail_q, tq);
}

__global__ void __launch_bounds__(256) risk_y_kernel(long long n, double *__restrict__ obj, const int *__restrict__ st, double var,
                                                     double denom) {
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < n; s += (long long)gridDim.x * 256) {
        if (st && st[s] != TWOSD_LP_OPTIMAL) continue;
        const double ex = __dadd_rn(obj[s], -var);
        obj[s] = __dadd_rn(var, __ddiv_rn(ex > 0.0 ? ex : 0.0, denom));
    }
}

// the grid of a kernel over n entries, `per` entries per block at full size; TWOSD_RISK_BLOCKS: the tests' knob
static int risk_grid(const twosd_ctx *c, long long n, int per, int cap) {
    long long g = std::min<long long>(std::max<long long>((n + per - 1) / per, 1), cap > 0 ? cap : 4 * c->num_cus);
    if (const char *e = getenv("TWOSD_RISK_BLOCKS")) g = std::max(1, std::min(atoi(e), 65535));   // the result must not change
    return (int)g;
}

int risk_select(twosd_ctx *c, long long n, const double *d_val, const double *d_w, const int *d_st, double scale, bool has_add,
                double add, double level, const char *who, RiskResult *out) {
    RiskState &S = c->risk;
    int rc;
    if ((rc = S.u64.fit(kRiskWords)) || (rc = S.part.fit(kRiskShards))) return rc;
    unsigned long long *hist = S.u64;
    RiskSel *sel = (RiskSel *)(S.u64 + kRiskHistWords);
    RiskIn I{n, d_val, d_w, d_st, scale, add, has_add ? 1 : 0};
    const int grid = risk_grid(c, n, 4096, 0);
    HIPCHK(hipEventRecord(c->ev[EV_MARK_0], c->stream));
    HIPCHK(hipMemsetAsync(S.u64, 0, sizeof(unsigned long long) * kRiskWords, c->stream));
    hipLaunchKernelGGL(risk_total_kernel, dim3(grid), dim3(256), 0, c->stream, I, sel);
    HIPCHK(hipGetLastError());
    RiskSel h{};
    HIPCHK(hipMemcpyAsync(&h, sel, sizeof(RiskSel), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out->n_bad = (long long)h.n_bad;
    out->n_ok = (long long)h.n_ok;
    out->total_q = h.total_q;
    out->tail_q = 0;
    out->var = out->cvar = NAN;
    if (h.n_ok == 0 || h.total_q == 0)
        return fail(TWOSD_E_ARG, "%s: no entry counts (%lld of %lld entries are optimal, their integer weights sum to %llu)", who,
                    (long long)h.n_ok, n, h.total_q);
    const unsigned long long t = risk_threshold(level, h.total_q);
    HIPCHK(hipMemcpyAsync(&sel->target, &t, sizeof t, hipMemcpyHostToDevice, c->stream));
    for (int p = 0; p < kRiskPasses; ++p) {
        hipLaunchKernelGGL(risk_hist_kernel, dim3(grid), dim3(256), 0, c->stream, I, p, sel, hist + (size_t)p * kRiskBins);
        hipLaunchKernelGGL(risk_pick_kernel, dim3(1), dim3(256), 0, c->stream, hist + (size_t)p * kRiskBins, sel);
    }
    hipLaunchKernelGGL(risk_tailsum_kernel, dim3(risk_grid(c, n, 4096, kRiskShards)), dim3(256), 0, c->stream, I, sel, S.part.p);
    HIPCHK(hipGetLastError());
    double part[kRiskShards];
    HIPCHK(hipMemcpyAsync(&h, sel, sizeof(RiskSel), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(part, S.part, sizeof part, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(c->ev[EV_MARK_1], c->stream));
    HIPCHK(hipEventSynchronize(c->ev[EV_MARK_1]));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[EV_MARK_0], c->ev[EV_MARK_1]);
    S.ms[0] = ms;
    double sum = 0.0;
    for (int b = 0; b < kRiskShards; ++b) sum = sum + part[b];
    const double var = risk_unkey(h.prefix);
    const double den = (1.0 - level) * (double)h.total_q;
    out->var = var;
    out->cvar = var + sum / den;
    out->tail_q = h.tail_q;
    return TWOSD_OK;
}

int risk_form_y(twosd_ctx *c, long long n, double *d_obj, const int *d_st, double var, double denom) {
    if (n <= 0) return TWOSD_OK;
    hipLaunchKernelGGL(risk_y_kernel, dim3(risk_grid(c, n, 2048, 0)), dim3(256), 0, c->stream, n, d_obj, d_st, var, denom);
    HIPCHK(hipGetLastError());
    return TWOSD_OK;
}

// ---- the tail cut ------------------------------------------------------------------------------
struct TailParams {
    int n, k, k4, nv, tpb, nchunks;   // tpb: 64-scenario tiles per shard
    int has_add;
    double scale, eta, add;
    const double *dv, *w, *PK, *val;
    const int *picks;
    double *slots;                    // nchunks x k
};

__device__ __forceinline__ bool tail_flag(const TailParams &P, int s) {
    const double v = P.val[s];
    return (P.has_add ? __dadd_rn(v, P.add) : v) > P.eta;
}

// out[0] += W_t, out[1] += the total (blockIdx.y == 0 only), hist[v] += the tail weight of pick v
// over the window of kRiskVW vertices blockIdx.y
__global__ void __launch_bounds__(1024) risk_thist_kernel(TailParams P, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long hl[kRiskVW];
    __shared__ unsigned long long tot[2];
    const int v0 = blockIdx.y * kRiskVW, v1 = min(P.nv, v0 + kRiskVW);
    for (int i = threadIdx.x; i < kRiskVW; i += 1024) hl[i] = 0ull;
    if (threadIdx.x < 2) tot[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long wt = 0, wa = 0;
    for (int s = blockIdx.x * 1024 + threadIdx.x; s < P.n; s += gridDim.x * 1024) {
        const unsigned long long q = reform_q(P.w[s], P.scale);
        if (!q) continue;
        wa += q;
        if (!tail_flag(P, s)) continue;
        wt += q;
        const int pick = P.picks[s];
        if (pick < v0 || pick >= v1) continue;
        __hip_atomic_fetch_add(&hl[pick - v0], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (blockIdx.y == 0) {
        for (int o = 32; o > 0; o >>= 1) { wt += __shfl_xor(wt, o); wa += __shfl_xor(wa, o); }
        if ((threadIdx.x & 63) == 0) {
            if (wt) __hip_atomic_fetch_add(&tot[0], wt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (wa) __hip_atomic_fetch_add(&tot[1], wa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    if (blockIdx.y == 0 && threadIdx.x < 2 && tot[threadIdx.x]) atomicAdd(&out[threadIdx.x], tot[threadIdx.x]);
    for (int i = threadIdx.x; i < v1 - v0; i += 1024) {
        const unsigned long long h = hl[i];
        if (h) atomicAdd(&out[2 + v0 + i], h);
    }
}

// slots[chunk][e] = sum over the chunk's tail scenarios of q PK[pick, e] dv[s, e]; KE elements per lane
template <int KE>
__global__ void __launch_bounds__(256) risk_treform_kernel(TailParams P) {
    __shared__ double comb[KE * 64];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ntiles = (P.n + 63) >> 6;
    int ec[KE];   // this lane's elements, clamped to k - 1 (a lane past k repeats the last: its sums are never stored)
#pragma unroll
    for (int u = 0; u < KE; ++u) ec[u] = min(lane + 64 * u, P.k - 1);
    for (int chunk = blockIdx.x; chunk < P.nchunks; chunk += gridDim.x) {
        const int t0 = chunk * P.tpb, t1 = min(ntiles, t0 + P.tpb);
        double acc[KE];
#pragma unroll
        for (int u = 0; u < KE; ++u) acc[u] = 0.0;
        for (int t = t0 + wid; t < t1; t += 4) {
            // lanes = the tile's scenarios
            const int s = t * 64 + lane;
            const bool valid = s < P.n;
            const int pick = valid ? P.picks[s] : -1;
            const bool ok = pick >= 0 && pick < P.nv && tail_flag(P, s);
            const double qf = ok ? (double)reform_q(P.w[s], P.scale) : 0.0;
            const int qlo = __double2loint(qf), qhi = __double2hiint(qf);
            const int pk0 = ok ? pick : 0;
            unsigned long long live = __ballot(qf != 0.0);
            const double *dvt = P.dv + (size_t)(t * 64) * P.k;
            // lanes = elements; the tail scenarios of the tile one at a time, lowest first
            while (live) {
                const int i = __builtin_ctzll(live);
                live &= live - 1;
                const int pv = __builtin_amdgcn_readlane(pk0, i);
                const double wq = __hiloint2double(__builtin_amdgcn_readlane(qhi, i), __builtin_amdgcn_readlane(qlo, i));
#pragma unroll
                for (int u = 0; u < KE; ++u)
                    acc[u] += wq * P.PK[(size_t)pv * P.k4 + ec[u]] * dvt[(size_t)i * P.k + ec[u]];
            }
        }
        // the block's four waves combined in wave order
        for (int wv = 0; wv < 4; ++wv) {
            if (wid == wv) {
#pragma unroll
                for (int u = 0; u < KE; ++u) {
                    double &d = comb[u * 64 + lane];
                    d = wv == 0 ? acc[u] : d + acc[u];
                }
            }
            __syncthreads();
        }
        for (int e = threadIdx.x; e < P.k; e += 256) P.slots[(size_t)chunk * P.k + e] = comb[e];
        __syncthreads();   // comb is the next chunk's
    }
}

// ---- tail handles: the tail of the last cut as a compact list ---------------------------------
// Order-preserving compaction, the same under any grid: a wave takes 64-scenario tiles; the tile's
// flags are one ballot.  Pass 1 writes the tiles' counts, one block scans them (exclusive; the total
// behind the last), pass 2 writes (scenario, pick) at the tile's offset plus the lane's rank among
// the flagged lanes below it.
struct TailKeep {
    int n, has_add;
    double eta, add;
    const double *val;
    const int *picks;
};

__device__ __forceinline__ bool keep_flag(const TailKeep &P, int s) {   // tail_flag, bit for bit
    const double v = P.val[s];
    return (P.has_add ? __dadd_rn(v, P.add) : v) > P.eta;
}

__global__ void __launch_bounds__(256) risk_tcount_kernel(TailKeep P, int *__restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int ntiles = (P.n + 63) >> 6;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < ntiles; t += gridDim.x * 4) {
        const int s = t * 64 + lane;
        const unsigned long long m = __ballot(s < P.n && keep_flag(P, s));
        if (lane == 0) cnt[t] = __popcll(m);
    }
}

// one block: cnt[t] <- sum_{u < t} cnt[u] for t < ntiles, cnt[ntiles] <- the total.  A thread owns a
// run of consecutive tiles; the 1024 runs' sums are scanned by thread 0.
__global__ void __launch_bounds__(1024) risk_tscan_kernel(int ntiles, int *__restrict__ cnt) {
    __shared__ int run[1024];
    const int per = (ntiles + 1023) / 1024;
    const int a = min(ntiles, (int)threadIdx.x * per), b = min(ntiles, a + per);
    int sum = 0;
    for (int t = a; t < b; ++t) sum += cnt[t];
    run[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int i = 0; i < 1024; ++i) { const int v = run[i]; run[i] = acc; acc += v; }
        cnt[ntiles] = acc;
    }
    __syncthreads();
    int off = run[threadIdx.x];
    for (int t = a; t < b; ++t) { const int v = cnt[t]; cnt[t] = off; off += v; }
}

__global__ void __launch_bounds__(256) risk_tscatter_kernel(TailKeep P, const int *__restrict__ offs, int *__restrict__ scen,
                                                            int *__restrict__ pick) {
    const int lane = threadIdx.x & 63;
    const int ntiles = (P.n + 63) >> 6;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < ntiles; t += gridDim.x * 4) {
        const int s = t * 64 + lane;
        const bool f = s < P.n && keep_flag(P, s);
        const unsigned long long m = __ballot(f);
        if (!f) continue;
        const int o = offs[t] + __popcll(m & ((1ull << lane) - 1ull));
        scen[o] = s;
        pick[o] = P.picks[s];
    }
}

// the last cut's state rule, and the two checks of a reader of the epigraph's weights
static int last_cut_of(twosd_ctx *c, int epi, const char *who) {
    if (int rc = cut_last_usable(c, epi, who, "read")) return rc;
    if (c->last_cut_n > c->epis[epi].count)
        return fail(TWOSD_E_STATE, "%s: the last cut holds %d scenarios, epigraph %d only %d", who, c->last_cut_n, epi,
                    c->epis[epi].count);
    if (!(c->epis[epi].total_weight > 0.0)) return fail(TWOSD_E_STATE, "%s: epigraph %d holds no scenario weight", who, epi);
    return TWOSD_OK;
}

}  // namespace twosd

using namespace twosd;

extern "C" int twosd_quantile_of_values(twosd_ctx *c, int64_t n, const double *values, const double *weights, const int *status,
                                        double level, double *var, double *cvar, uint64_t *tail_q, uint64_t *total_q,
                                        int64_t *n_bad) {
    if (!c) return fail(TWOSD_E_STATE, "quantile_of_values: no context");
    if (!values || n < 1 || n > (1ll << 27))
        return fail(TWOSD_E_ARG, "quantile_of_values: n = %lld outside [1, 2^27] or values NULL", (long long)n);
    if (!(level > 0.0 && level < 1.0)) return fail(TWOSD_E_ARG, "quantile_of_values: level = %g outside (0, 1)", level);
    double total = 0.0;
    if (weights) {
        for (int64_t s = 0; s < n; ++s) {
            if (!(weights[s] >= 0.0) || !std::isfinite(weights[s]))
                return fail(TWOSD_E_ARG, "quantile_of_values: weight %lld is %g (finite and >= 0)", (long long)s, weights[s]);
            total = total + weights[s];   // index order, as an epigraph accumulates its total
        }
        if (!(total > 0.0) || !std::isfinite(total)) return fail(TWOSD_E_ARG, "quantile_of_values: no entry counts (the weights sum to %g)", total);
    }
    HIPCHK(hipSetDevice(c->device));
    RiskState &S = c->risk;
    int rc;
    if ((rc = S.val.grow((size_t)n, 0, c->stream))) return rc;
    HIPCHK(hipMemcpy(S.val, values, sizeof(double) * n, hipMemcpyHostToDevice));
    if (weights) {
        if ((rc = S.w.grow((size_t)n, 0, c->stream))) return rc;
        HIPCHK(hipMemcpy(S.w, weights, sizeof(double) * n, hipMemcpyHostToDevice));
    }
    if (status) {
        if ((rc = S.st.grow((size_t)n, 0, c->stream))) return rc;
        HIPCHK(hipMemcpy(S.st, status, sizeof(int) * n, hipMemcpyHostToDevice));
    }
    RiskResult R{};
    rc = risk_select(c, n, S.val, weights ? S.w.p : nullptr, status ? S.st.p : nullptr, weights ? kReformFix / total : 1.0, false, 0.0,
                     level, "quantile_of_values", &R);
    if (n_bad) *n_bad = R.n_bad;
    if (total_q) *total_q = R.total_q;
    if (rc) return rc;
    if (var) *var = R.var;
    if (cvar) *cvar = R.cvar;
    if (tail_q) *tail_q = R.tail_q;
    return TWOSD_OK;
}

extern "C" int twosd_cut_quantile(twosd_ctx *c, int epi, double level, double *var, double *cvar, double *tail_weight,
                                  double *total_weight) {
    int rc = last_cut_of(c, epi, "cut_quantile");
    if (rc) return rc;
    if (!(level > 0.0 && level < 1.0)) return fail(TWOSD_E_ARG, "cut_quantile: level = %g outside (0, 1)", level);
    HIPCHK(hipSetDevice(c->device));
    const EpiDevice &E = c->epis[epi];
    RiskResult R{};
    if ((rc = risk_select(c, c->last_cut_n, cut_last_val(c), E.d_w, nullptr, kReformFix / E.total_weight, c->has_bounds, c->c0, level,
                          "cut_quantile", &R)))
        return rc;
    const double wunit = E.total_weight / kReformFix;
    if (var) *var = R.var;
    if (cvar) *cvar = R.cvar;
    if (tail_weight) *tail_weight = (double)R.tail_q * wunit;
    if (total_weight) *total_weight = (double)R.total_q * wunit;
    return TWOSD_OK;
}

extern "C" int twosd_cut_tail(twosd_ctx *c, int epi, double eta, double *alpha, double *beta, double *tail_weight,
                              double *total_weight) {
    if (c && c->has_template && c->k > 127)   // before the state rule: no cut of such a template exists
        return fail(TWOSD_E_UNSUPPORTED, "k = %d random elements exceeds the cut kernel envelope (127)", c->k);
    int rc = last_cut_of(c, epi, "cut_tail");
    if (rc) return rc;
    if (!alpha || (c->n1 > 0 && !beta)) return fail(TWOSD_E_ARG, "cut_tail: alpha/beta NULL");
    if (std::isnan(eta)) return fail(TWOSD_E_ARG, "cut_tail: eta is NaN");
    HIPCHK(hipSetDevice(c->device));
    const EpiDevice &E = c->epis[epi];
    RiskState &S = c->risk;
    ReformState &R = c->reform;   // one handle, one row: its scratch, its S sums (f64) and its output row 0
    const int n = c->last_cut_n, nv = c->last_cut_nv, k = c->k, n1 = c->n1;
    const double *PK = nullptr;
    int k4 = 0;
    const ReformShards sh = reform_shards(n);   // n >= 1: last_cut_of
    if ((rc = cut_pk_current(c, &PK, &k4)) || (rc = reform_prepare(c, 1, 1, nv)) || (rc = S.thist.fit((size_t)2 + nv)) ||
        (rc = R.slots.fit((size_t)sh.nchunks * std::max(k, 1))) || (rc = R.f64.fit(std::max(k, 1))))
        return rc;
    const double wunit = E.total_weight / kReformFix;
    TailParams P{};
    P.n = n; P.k = k; P.k4 = k4; P.nv = nv; P.tpb = sh.tpb; P.nchunks = sh.nchunks;
    P.has_add = c->has_bounds ? 1 : 0; P.add = c->c0; P.eta = eta; P.scale = kReformFix / E.total_weight;
    P.dv = E.d_dv; P.w = E.d_w; P.PK = PK; P.val = cut_last_val(c); P.picks = cut_last_arg(c);
    P.slots = R.slots;
    HIPCHK(hipEventRecord(c->ev[EV_MARK_0], c->stream));
    HIPCHK(hipMemsetAsync(S.thist, 0, sizeof(unsigned long long) * ((size_t)2 + nv), c->stream));
    hipLaunchKernelGGL(risk_thist_kernel, dim3(risk_grid(c, n, 8192, 64), (nv + kRiskVW - 1) / kRiskVW), dim3(1024), 0, c->stream, P,
                       S.thist.p);
    if (k > 0) {
        const dim3 rgrid(std::min(sh.nchunks, risk_grid(c, n, 256, sh.nchunks)));
        if (k <= 64) hipLaunchKernelGGL(risk_treform_kernel<1>, rgrid, dim3(256), 0, c->stream, P);
        else hipLaunchKernelGGL(risk_treform_kernel<2>, rgrid, dim3(256), 0, c->stream, P);
        reform_sum_shards(c, false, sh.nchunks, k, R.slots.p, R.f64.p);   // plain shard order
    }
    // W_t is the one W word; the per-vertex weights follow the two totals (row 0: the stride is not read)
    if ((rc = reform_finalize_block(c, 1, 1, 0, nv, nv, S.thist + 2, R.f64.p, S.thist.p, wunit))) return rc;
    std::vector<double> out((size_t)2 + n1);   // one row: [alpha][weight_mark][beta], one copy
    unsigned long long tw[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(out.data(), R.out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(tw, S.thist, sizeof tw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(c->ev[EV_MARK_1], c->stream));
    HIPCHK(hipEventSynchronize(c->ev[EV_MARK_1]));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[EV_MARK_0], c->ev[EV_MARK_1]);
    S.ms[1] = ms;
    *alpha = out[0];
    for (int j = 0; j < n1; ++j) beta[j] = out[2 + j];
    if (tail_weight) *tail_weight = (double)tw[0] * wunit;
    if (total_weight) *total_weight = (double)tw[1] * wunit;
    return TWOSD_OK;
}

extern "C" int twosd_tail_keep(twosd_ctx *c, int epi, double eta, int *handle) {
    if (c && c->has_template && c->k > 127)   // as twosd_cut_tail: no cut of such a template exists
        return fail(TWOSD_E_UNSUPPORTED, "k = %d random elements exceeds the cut kernel envelope (127)", c->k);
    int rc = last_cut_of(c, epi, "tail_keep");
    if (rc) return rc;
    if (!handle) return fail(TWOSD_E_ARG, "tail_keep: handle is NULL");
    if (std::isnan(eta)) return fail(TWOSD_E_ARG, "tail_keep: eta is NaN");
    HIPCHK(hipSetDevice(c->device));
    RiskState &S = c->risk;
    const int n = c->last_cut_n, ntiles = (n + 63) >> 6;
    if ((rc = S.tcnt.fit((size_t)ntiles + 1))) return rc;
    TailKeep P{};
    P.n = n; P.has_add = c->has_bounds ? 1 : 0; P.add = c->c0; P.eta = eta;
    P.val = cut_last_val(c); P.picks = cut_last_arg(c);
    const dim3 grid(risk_grid(c, n, 256, 0));
    HIPCHK(hipEventRecord(c->ev[EV_MARK_0], c->stream));
    hipLaunchKernelGGL(risk_tcount_kernel, grid, dim3(256), 0, c->stream, P, S.tcnt.p);
    hipLaunchKernelGGL(risk_tscan_kernel, dim3(1), dim3(1024), 0, c->stream, ntiles, S.tcnt.p);
    HIPCHK(hipGetLastError());
    int nt = 0;   // the one copy: it sizes the handle's two arrays
    HIPCHK(hipMemcpyAsync(&nt, S.tcnt + ntiles, sizeof nt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (nt < 0 || nt > n) return fail(TWOSD_E_DEVICE, "tail_keep: the tiles' counts sum to %d of %d scenarios", nt, n);
    PickSet fresh;
    if ((rc = fresh.d.alloc((size_t)nt)) || (rc = fresh.scen.alloc((size_t)nt))) return rc;
    if (nt > 0) {
        hipLaunchKernelGGL(risk_tscatter_kernel, grid, dim3(256), 0, c->stream, P, S.tcnt.p, fresh.scen.p, fresh.d.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(c->ev[EV_MARK_1], c->stream));
    HIPCHK(hipEventSynchronize(c->ev[EV_MARK_1]));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[EV_MARK_0], c->ev[EV_MARK_1]);
    S.keep_ms = ms;
    fresh.epi = epi; fresh.n = n; fresh.nv = c->last_cut_nv; fresh.nt = nt; fresh.eta = eta; fresh.live = true;
    int id = 0;
    *pick_slot(c, &id) = std::move(fresh);
    *handle = id;
    return TWOSD_OK;
}

// a usable tail handle of the shared table, or the error with its message
static int usable_tail(twosd_ctx *c, int handle, const char *what, PickSet **out) {
    int rc = usable_pick(c, handle, what, out);
    if (rc) return rc;
    if (!(*out)->is_tail())
        return fail(TWOSD_E_ARG, "%s: handle %d is a pick handle, not a tail handle (twosd_picks_info / twosd_picks_get)", what, handle);
    return TWOSD_OK;
}

extern "C" int twosd_tail_info(twosd_ctx *c, int handle, int *epi, int *n, int *nv, int *nt, double *eta) {
    if (!c) return fail(TWOSD_E_ARG, "tail_info: ctx is NULL");
    PickSet *h = nullptr;
    int rc = usable_tail(c, handle, "tail_info", &h);
    if (rc) return rc;
    if (epi) *epi = h->epi;
    if (n) *n = h->n;
    if (nv) *nv = h->nv;
    if (nt) *nt = h->nt;
    if (eta) *eta = h->eta;
    return TWOSD_OK;
}

extern "C" int twosd_tail_get(twosd_ctx *c, int handle, int *scen, int *pick) {
    if (!c) return fail(TWOSD_E_ARG, "tail_get: ctx is NULL");
    PickSet *h = nullptr;
    int rc = usable_tail(c, handle, "tail_get", &h);
    if (rc) return rc;
    if (h->nt == 0) return TWOSD_OK;
    if (!scen || !pick) return fail(TWOSD_E_ARG, "tail_get: scen / pick NULL for a tail of %d scenarios", h->nt);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(scen, h->scen, sizeof(int) * h->nt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(pick, h->d, sizeof(int) * h->nt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return TWOSD_OK;
}

extern "C" int twosd_tail_last_ms(twosd_ctx *c, double *ms) {
    if (!c || !ms) return fail(TWOSD_E_ARG, "tail_last_ms: NULL");
    *ms = c->risk.keep_ms;
    return TWOSD_OK;
}

extern "C" int twosd_risk_last_ms(twosd_ctx *c, double *ms2) {
    if (!c || !ms2) return fail(TWOSD_E_ARG, "risk_last_ms: NULL");
    ms2[0] = c->risk.ms[0];
    ms2[1] = c->risk.ms[1];
    return TWOSD_OK;
}
