// evaluate.hip -- out-of-sample evaluation at x on device-drawn scenarios: the moments kernels and
// their merge, the chunked sample-and-solve loop under a sampling plan, twosd_evaluate_* and
// twosd_moments_*.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "twosd_internal.h"
#include "twosd_ctx.h"

using namespace twosd;

// Sample moments of a batch's objectives (twosd_moments per block): block b owns the contiguous
// range [b L, min(N, (b + 1) L)), L = ceil(N / kMomBlocks), so a block's record is the moments of
// a slice of the stream and the host merges the records in block order (twosd_moments_merge).
// An entry counts when its status is optimal (PAIRED: in both arrays); the value of any other
// entry is never loaded.  Per block, over its counted entries:
//   0. the first counted index (each thread stops at its first; tree min) gives the pivot K = v[first]
//   1. n and S = sum (v - K): mean = K + S / n.  The pivot keeps the sum at the size of the
//      spread, not of the values, and makes a constant slice exact (S = 0, mean = K, m2 = 0)
//   2. sum (v - mean)^2, min, max -- the second read of the slice comes from L2
// never the one-pass sum v^2 - n mean^2, which loses 2 log10(mean / sd) digits.  PAIRED adds the
// records of b and of the per-scenario difference d = a - b (formed per entry, then reduced like
// a value): part[3 blk + 0 / 1 / 2] = a, b, d.  Every reduction is the fixed LDS tree of
// lp_obj_kernel over per-thread partials of a fixed stride: no atomics, the same bits on every run.
constexpr int kMomBlocks = 256;
template <typename T, typename Op>
__device__ __forceinline__ T mom_block_reduce(T v, T *sh, Op op) {
    __syncthreads();   // sh may still be read as the previous reduction's result
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = op(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    return sh[0];
}
template <bool PAIRED>
__global__ void __launch_bounds__(256) eval_moments_kernel(long long N, const double *__restrict__ va,
                                                           const int *__restrict__ sa, const double *__restrict__ vb,
                                                           const int *__restrict__ sb, twosd_moments *__restrict__ part) {
    constexpr int R = PAIRED ? 3 : 1;
    __shared__ double shd[256];
    __shared__ long long shi[256];
    const long long L = (N + kMomBlocks - 1) / kMomBlocks;
    const long long lo0 = (long long)blockIdx.x * L, lo = lo0 < N ? lo0 : N, hi = lo + L < N ? lo + L : N;
    const auto counted = [&](long long i) {
        return (!sa || sa[i] == TWOSD_LP_OPTIMAL) && (!PAIRED || !sb || sb[i] == TWOSD_LP_OPTIMAL);
    };
    const auto add = [](auto x, auto y) { return x + y; };
    const long long none = 0x7fffffffffffffffLL;
    long long first = none;
    for (long long i = lo + threadIdx.x; i < hi; i += 256)
        if (counted(i)) { first = i; break; }
    first = mom_block_reduce(first, shi, [](long long x, long long y) { return x < y ? x : y; });
    twosd_moments *out = part + (size_t)R * blockIdx.x;
    if (first == none) {   // an empty slice, or nothing counted: the merge's identity
        if (threadIdx.x == 0)
            for (int r = 0; r < R; ++r) out[r] = twosd_moments{0, hi - lo, 0.0, 0.0, HUGE_VAL, -HUGE_VAL};
        return;
    }
    double K[R], S[R], mean[R], q[R], mn[R], mx[R];
    K[0] = va[first];
    if (PAIRED) { K[1] = vb[first]; K[2] = K[0] - K[1]; }
    long long n = 0;
    for (int r = 0; r < R; ++r) S[r] = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        if (!counted(i)) continue;
        ++n;
        const double a = va[i];
        S[0] += a - K[0];
        if (PAIRED) {
            const double b = vb[i];
            S[1] += b - K[1];
            S[2] += (a - b) - K[2];
        }
    }
    n = mom_block_reduce(n, shi, add);
    for (int r = 0; r < R; ++r) {
        S[r] = mom_block_reduce(S[r], shd, add);
        mean[r] = K[r] + S[r] / (double)n;
        q[r] = 0.0; mn[r] = HUGE_VAL; mx[r] = -HUGE_VAL;
    }
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        if (!counted(i)) continue;
        double v[R];
        v[0] = va[i];
        if (PAIRED) { v[1] = vb[i]; v[2] = v[0] - v[1]; }
        for (int r = 0; r < R; ++r) {
            const double e = v[r] - mean[r];
            q[r] = fma(e, e, q[r]);
            mn[r] = v[r] < mn[r] ? v[r] : mn[r];
            mx[r] = v[r] > mx[r] ? v[r] : mx[r];
        }
    }
    for (int r = 0; r < R; ++r) {
        q[r] = mom_block_reduce(q[r], shd, add);
        mn[r] = mom_block_reduce(mn[r], shd, [](double x, double y) { return x < y ? x : y; });
        mx[r] = mom_block_reduce(mx[r], shd, [](double x, double y) { return x > y ? x : y; });
    }
    if (threadIdx.x == 0)
        for (int r = 0; r < R; ++r) out[r] = twosd_moments{n, (hi - lo) - n, mean[r], n > 1 ? q[r] : 0.0, mn[r], mx[r]};
}

// Group means of a variance-reduced stream (twosd_sampling): the members of a
// group of G consecutive entries are dependent, so the moments are taken over the groups' means.
// One thread per group: status[b] = optimal iff all G entries are (else the first other status),
// and only then mean[b] = K + (sum_{i < G} (v[i] - K)) / G with K = v[0], the sum in index order
// from 0.0 -- a fixed order whatever the launch shape, the pivot keeping the sum at the size of the
// spread.  The values of a group left out are never loaded (they may be NaN); its mean reads 0.
// The means are stored relative to the chunk's pivot K0 = v[0] (0 when entry 0 is not optimal or
// not finite), mean[b] = m_b - K0, and *pivot = K0: the moments kernel's block records then merge
// at the size of the spread, not of the values (the merge's d d term loses 2^-53 |mean| / sd per
// step), and the host adds K0 back to mean, min and max.  m_b - K0 is exact, and min / max the
// means' own bits, whenever m_b / 2 <= K0 <= 2 m_b.
// The paired form runs it on each array: a group counts when it is optimal in both, which the
// moments kernel sees from the two group statuses, and it forms the difference of the means itself.
__global__ void __launch_bounds__(256) group_means_kernel(long long ngroups, int G, const double *__restrict__ v,
                                                          const int *__restrict__ st, double *__restrict__ mean,
                                                          int *__restrict__ gst, double *__restrict__ pivot) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= ngroups) return;
    const double K0 = ((!st || st[0] == TWOSD_LP_OPTIMAL) && isfinite(v[0])) ? v[0] : 0.0;
    if (b == 0) *pivot = K0;
    const long long lo = b * G;
    int bad = TWOSD_LP_OPTIMAL;
    if (st)
        for (int i = 0; i < G && bad == TWOSD_LP_OPTIMAL; ++i) bad = st[lo + i];
    double m = 0.0;
    if (bad == TWOSD_LP_OPTIMAL) {
        const double K = v[lo];
        double s = 0.0;
        for (int i = 0; i < G; ++i) s = __dadd_rn(s, __dadd_rn(v[lo + i], -K));
        m = __dadd_rn(__dadd_rn(K, __ddiv_rn(s, (double)G)), -K0);
    }
    mean[b] = m;
    gst[b] = bad;
}

// ---- out-of-sample moments (twosd_moments_*, twosd_evaluate_moments / _paired / _ci) --------------
static const twosd_moments kMomentsEmpty = {0, 0, 0.0, 0.0, HUGE_VAL, -HUGE_VAL};

// The pairwise update of Chan, Golub and LeVeque: the one merge of the blocks' records, of the
// chunks, of the batches and of the ranks.
extern "C" int twosd_moments_merge(const twosd_moments *a, const twosd_moments *b, twosd_moments *out) {
    if (!a || !b || !out) return fail(TWOSD_E_ARG, "moments_merge: NULL");
    const twosd_moments A = *a, B = *b;   // out may alias either
    if (A.n < 0 || B.n < 0) return fail(TWOSD_E_ARG, "moments_merge: negative count");
    twosd_moments r;
    if (B.n == 0) r = A;
    else if (A.n == 0) r = B;
    else {
        const double na = (double)A.n, nb = (double)B.n, n = (double)(A.n + B.n);
        const double d = B.mean - A.mean;
        r.n = A.n + B.n;
        r.mean = A.mean + d * (nb / n);
        r.m2 = A.m2 + B.m2 + d * d * (na * nb / n);
        r.min = B.min < A.min ? B.min : A.min;
        r.max = B.max > A.max ? B.max : A.max;
    }
    r.n_bad = A.n_bad + B.n_bad;
    *out = r;
    return TWOSD_OK;
}

// moments of N device-resident values (PAIRED: also of vb and of va - vb) into out[0 .. R): the
// kernel's kMomBlocks records, one small copy, one stream sync, merged in block order
static int device_moments(twosd_ctx *c, long long N, const double *d_va, const int *d_sa, const double *d_vb,
                          const int *d_sb, twosd_moments *out) {
    const int R = d_vb ? 3 : 1;
    for (int r = 0; r < R; ++r) out[r] = kMomentsEmpty;
    if (N <= 0) return TWOSD_OK;
    if (!c->d_mompart)
        if (int rc = c->d_mompart.alloc(sizeof(twosd_moments) * 3 * kMomBlocks)) return rc;
    twosd_moments *d_part = (twosd_moments *)c->d_mompart.p;
    if (d_vb)
        hipLaunchKernelGGL(eval_moments_kernel<true>, dim3(kMomBlocks), dim3(256), 0, c->stream, N, d_va, d_sa, d_vb, d_sb, d_part);
    else
        hipLaunchKernelGGL(eval_moments_kernel<false>, dim3(kMomBlocks), dim3(256), 0, c->stream, N, d_va, d_sa, d_vb, d_sb, d_part);
    HIPCHK(hipGetLastError());
    std::vector<twosd_moments> part((size_t)R * kMomBlocks);
    HIPCHK(hipMemcpyAsync(part.data(), d_part, sizeof(twosd_moments) * part.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int b = 0; b < kMomBlocks; ++b)
        for (int r = 0; r < R; ++r) twosd_moments_merge(&out[r], &part[(size_t)R * b + r], &out[r]);
    return TWOSD_OK;
}

// device_moments over the means of groups of G consecutive entries (N a multiple of G; G = 1: the
// entries themselves): group_means_kernel into the context's group buffers, then the moments
// kernel unchanged on the N / G means and group statuses
static int device_moments_grouped(twosd_ctx *c, long long N, int G, const double *d_va, const int *d_sa, const double *d_vb,
                                  const int *d_sb, twosd_moments *out) {
    if (G <= 1 || N <= 0) return device_moments(c, N, d_va, d_sa, d_vb, d_sb, out);
    const long long ng = N / G;
    const int R = d_vb ? 2 : 1;
    int rc;
    if ((rc = c->d_gm_mean.fit((size_t)R * ng + 2)) || (rc = c->d_gm_st.fit((size_t)R * ng))) return rc;   // + the two pivots
    double *d_piv = c->d_gm_mean + (size_t)R * ng;
    const unsigned nb = (unsigned)((ng + 255) / 256);
    hipLaunchKernelGGL(group_means_kernel, dim3(nb), dim3(256), 0, c->stream, ng, G, d_va, d_sa, c->d_gm_mean.p, c->d_gm_st.p, d_piv);
    HIPCHK(hipGetLastError());
    if (d_vb) {
        hipLaunchKernelGGL(group_means_kernel, dim3(nb), dim3(256), 0, c->stream, ng, G, d_vb, d_sb, c->d_gm_mean + ng,
                           c->d_gm_st + ng, d_piv + 1);
        HIPCHK(hipGetLastError());
    }
    double piv[2] = {0.0, 0.0};
    HIPCHK(hipMemcpyAsync(piv, d_piv, sizeof(double) * (d_vb ? 2 : 1), hipMemcpyDeviceToHost, c->stream));   // device_moments drains the stream
    if ((rc = device_moments(c, ng, c->d_gm_mean, c->d_gm_st, d_vb ? c->d_gm_mean + ng : nullptr, d_vb ? c->d_gm_st + ng : nullptr, out)))
        return rc;
    const double back[3] = {piv[0], piv[1], piv[0] - piv[1]};   // the difference record is of (a - K0a) - (b - K0b)
    for (int r = 0; r < (d_vb ? 3 : 1); ++r)
        if (out[r].n > 0) { out[r].mean += back[r]; out[r].min += back[r]; out[r].max += back[r]; }
    return TWOSD_OK;
}

static int moments_of_values(twosd_ctx *c, int64_t n, int G, const double *obj, const int *status, twosd_moments *out) {
    if (!c) return fail(TWOSD_E_STATE, "moments_of_values: no context");
    if (!out || n < 0 || (n > 0 && !obj)) return fail(TWOSD_E_ARG, "moments_of_values: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if (n > 0) {
        if ((rc = c->d_ev_obj.grow((size_t)n, 0, c->stream))) return rc;
        HIPCHK(hipMemcpy(c->d_ev_obj, obj, sizeof(double) * n, hipMemcpyHostToDevice));
        if (status) {
            if ((rc = c->d_ev_st.grow((size_t)n, 0, c->stream))) return rc;
            HIPCHK(hipMemcpy(c->d_ev_st, status, sizeof(int) * n, hipMemcpyHostToDevice));
        }
    }
    return device_moments_grouped(c, n, G, c->d_ev_obj, status ? c->d_ev_st : nullptr, nullptr, nullptr, out);
}

extern "C" int twosd_moments_of_values(twosd_ctx *c, int64_t n, const double *obj, const int *status, twosd_moments *out) {
    return moments_of_values(c, n, 1, obj, status, out);
}

extern "C" int twosd_moments_of_values_grouped(twosd_ctx *c, int64_t n, int G, const double *obj, const int *status,
                                               twosd_moments *out) {
    if (G < 1 || G > 256) return fail(TWOSD_E_ARG, "moments_of_values_grouped: need 1 <= G <= 256, not %d", G);
    if (n > 0 && n % G) return fail(TWOSD_E_ARG, "moments_of_values_grouped: n = %lld is no multiple of G = %d", (long long)n, G);
    return moments_of_values(c, n, G, obj, status, out);
}

// scenarios per evaluate chunk; for a plan with G > 1 rounded down to whole groups (at least one)
static int64_t eval_chunk_size(int G) {
    int64_t chunk = 1 << 20;
    if (const char *e = getenv("TWOSD_EVAL_CHUNK")) chunk = std::min<int64_t>(std::max<int64_t>(atoll(e), 1), 1 << 24);   // test hook
    if (G > 1) chunk = std::max<int64_t>(chunk / G * G, G);
    return chunk;
}

// the sampling plan of an evaluate call: (mode, group) of twosd_sampling, i.i.d. by default
struct EvalPlan { int mode = TWOSD_SAMPLING_IID, G = 1; };

// scenarios [at, at + n) of stream `seed` drawn into d_dvtmp and solved at x; copy_lp_outputs adds
// the bounds' constant to d_obj and keeps the last-LP statistics current; obj (host, nullable)
// receives the objectives, nothing else is copied out.  The i.i.d. plan launches sample_kernel itself.
// TWOSD_OK, or TWOSD_E_LP with d_obj / d_status still set, or a failure.
static int eval_solve_chunk(twosd_ctx *c, const double *x, int64_t at, int n, uint64_t seed, const EvalPlan &pl,
                            double *obj = nullptr) {
    int rc;
    if ((rc = c->d_dvtmp.grow((size_t)n * std::max(c->k, 1), 0, c->stream))) return rc;
    if ((rc = draw_scenarios(c, n, seed, (uint64_t)at, c->d_dvtmp, pl.mode, pl.G))) return rc;
    if ((rc = run_lp(c, x, c->d_dvtmp, n))) return rc;
    return copy_lp_outputs(c, n, obj, nullptr, nullptr, nullptr, nullptr);
}

static int eval_check_state(twosd_ctx *c, const char *who) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "%s: no template", who);
    if (!c->bp.has_basis) return fail(TWOSD_E_STATE, "%s: no warm-start basis", who);
    if (!c->has_dist) return fail(TWOSD_E_STATE, "%s: no distributions (twosd_set_distributions)", who);
    return TWOSD_OK;
}

// moments over [first, first + count) at xa (xb: the paired form, out[0 .. 3) = a, b, a - b);
// *lp_bad: some LP was not optimal (counted in n_bad; not a failure here).  Under a plan with
// G > 1 (first and count whole groups) the moments are of the group means, n / n_bad in groups.
static int eval_moments_range(twosd_ctx *c, const double *xa, const double *xb, int64_t first, int64_t count, uint64_t seed,
                              twosd_moments *out, bool *lp_bad, const EvalPlan &pl = EvalPlan()) {
    const int R = xb ? 3 : 1;
    const int64_t chunk = eval_chunk_size(pl.G);
    for (int r = 0; r < R; ++r) out[r] = kMomentsEmpty;
    for (int64_t at = 0; at < count; at += chunk) {
        const int n = (int)std::min(chunk, count - at);
        int rc = eval_solve_chunk(c, xa, first + at, n, seed, pl);
        if (rc == TWOSD_E_LP) *lp_bad = true;
        else if (rc) return rc;
        twosd_moments m[3];
        if (xb) {
            if ((rc = c->d_ev_obj.grow((size_t)n, 0, c->stream)) ||
                (rc = c->d_ev_st.grow((size_t)n, 0, c->stream)))
                return rc;
            HIPCHK(hipMemcpyAsync(c->d_ev_obj, c->d_obj, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(c->d_ev_st, c->d_status, sizeof(int) * n, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));   // the next solve may reallocate d_obj / d_status
            rc = eval_solve_chunk(c, xb, first + at, n, seed, pl);
            if (rc == TWOSD_E_LP) *lp_bad = true;
            else if (rc) return rc;
            if ((rc = device_moments_grouped(c, n, pl.G, c->d_ev_obj, c->d_ev_st, c->d_obj, c->d_status, m))) return rc;
        } else if ((rc = device_moments_grouped(c, n, pl.G, c->d_obj, c->d_status, nullptr, nullptr, m)))
            return rc;
        for (int r = 0; r < R; ++r) twosd_moments_merge(&out[r], &m[r], &out[r]);
    }
    return TWOSD_OK;
}

static int eval_lp_result(bool lp_bad, const twosd_moments &m, const char *who, int G = 1) {
    if (!lp_bad) return TWOSD_OK;
    if (G > 1)
        return fail(TWOSD_E_LP, "%s: %lld of %lld scenario groups hold an LP that is not optimal (left out of the moments, see n_bad)",
                    who, (long long)m.n_bad, (long long)(m.n + m.n_bad));
    return fail(TWOSD_E_LP, "%s: %lld of %lld scenario LPs not optimal (left out of the moments, see n_bad)", who,
                (long long)m.n_bad, (long long)(m.n + m.n_bad));
}

// the plan of an evaluate call, with `first` and `count` checked for whole groups
static int eval_plan(const twosd_sampling *plan, const char *who, int64_t first, int64_t count, const char *count_name,
                     EvalPlan *pl) {
    int rc;
    if ((rc = sampling_plan(plan, who, &pl->mode, &pl->G))) return rc;
    if (first >= 0 && (rc = whole_groups(who, "first", (unsigned long long)first, pl->G))) return rc;
    if (count >= 0 && (rc = whole_groups(who, count_name, (unsigned long long)count, pl->G))) return rc;
    return TWOSD_OK;
}

static int evaluate_moments(twosd_ctx *c, const double *x, int64_t first, int64_t count, uint64_t seed, twosd_moments *out,
                            const EvalPlan &pl) {
    int rc = eval_check_state(c, "evaluate_moments");
    if (rc) return rc;
    if (!out || first < 0 || count < 0 || (c->n1 > 0 && !x)) return fail(TWOSD_E_ARG, "evaluate_moments: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    bool lp_bad = false;
    if ((rc = eval_moments_range(c, x, nullptr, first, count, seed, out, &lp_bad, pl))) return rc;
    return eval_lp_result(lp_bad, *out, "evaluate_moments", pl.G);
}

extern "C" int twosd_evaluate_moments(twosd_ctx *c, const double *x, int64_t first, int64_t count, uint64_t seed,
                                      twosd_moments *out) {
    return evaluate_moments(c, x, first, count, seed, out, EvalPlan());
}

extern "C" int twosd_evaluate_moments_vr(twosd_ctx *c, const double *x, int64_t first, int64_t count, uint64_t seed,
                                         twosd_moments *out, const twosd_sampling *plan) {
    EvalPlan pl;
    if (int rc = eval_plan(plan, "evaluate_moments", first, count, "count", &pl)) return rc;
    return evaluate_moments(c, x, first, count, seed, out, pl);
}

static int evaluate_paired(twosd_ctx *c, const double *xa, const double *xb, int64_t first, int64_t count, uint64_t seed,
                           twosd_moments *a, twosd_moments *b, twosd_moments *diff, const EvalPlan &pl) {
    int rc = eval_check_state(c, "evaluate_paired");
    if (rc) return rc;
    if (!a || !b || !diff || first < 0 || count < 0 || !xa || !xb) return fail(TWOSD_E_ARG, "evaluate_paired: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    bool lp_bad = false;
    twosd_moments m[3];
    if ((rc = eval_moments_range(c, xa, xb, first, count, seed, m, &lp_bad, pl))) return rc;
    *a = m[0]; *b = m[1]; *diff = m[2];
    return eval_lp_result(lp_bad, m[0], "evaluate_paired", pl.G);
}

extern "C" int twosd_evaluate_paired(twosd_ctx *c, const double *xa, const double *xb, int64_t first, int64_t count,
                                     uint64_t seed, twosd_moments *a, twosd_moments *b, twosd_moments *diff) {
    return evaluate_paired(c, xa, xb, first, count, seed, a, b, diff, EvalPlan());
}

extern "C" int twosd_evaluate_paired_vr(twosd_ctx *c, const double *xa, const double *xb, int64_t first, int64_t count,
                                        uint64_t seed, twosd_moments *a, twosd_moments *b, twosd_moments *diff,
                                        const twosd_sampling *plan) {
    EvalPlan pl;
    if (int rc = eval_plan(plan, "evaluate_paired", first, count, "count", &pl)) return rc;
    return evaluate_paired(c, xa, xb, first, count, seed, a, b, diff, pl);
}

static int evaluate_ci(twosd_ctx *c, const double *x, uint64_t seed, int64_t first, int64_t batch, int64_t n_max, double z,
                       double rel_tol, double abs_tol, double offset, twosd_moments *out, double *half_width, int *converged,
                       const EvalPlan &pl) {
    if (!out || !half_width || !converged || first < 0) return fail(TWOSD_E_ARG, "evaluate_ci: bad arguments");
    if (batch < 2 || n_max < batch) return fail(TWOSD_E_ARG, "evaluate_ci: need 2 <= batch <= n_max (batch %lld, n_max %lld)", (long long)batch, (long long)n_max);
    if (!(z > 0.0) || !(rel_tol >= 0.0) || !(abs_tol >= 0.0) || !std::isfinite(offset))
        return fail(TWOSD_E_ARG, "evaluate_ci: need z > 0, tolerances >= 0 and a finite offset");
    int rc = eval_check_state(c, "evaluate_ci");
    if (rc) return rc;
    if (c->n1 > 0 && !x) return fail(TWOSD_E_ARG, "evaluate_ci: x required");
    HIPCHK(hipSetDevice(c->device));
    twosd_moments acc = kMomentsEmpty;
    bool lp_bad = false;
    double hw = HUGE_VAL;
    int conv = 0;
    for (int64_t done = 0; done < n_max && !conv; ) {
        const int64_t cnt = std::min(batch, n_max - done);
        twosd_moments m;
        if ((rc = eval_moments_range(c, x, nullptr, first + done, cnt, seed, &m, &lp_bad, pl))) return rc;
        twosd_moments_merge(&acc, &m, &acc);
        done += cnt;
        if (acc.n >= 2) {
            hw = z * std::sqrt(acc.m2 / (double)(acc.n - 1) / (double)acc.n);
            conv = hw <= std::max(abs_tol, rel_tol * std::fabs(offset + acc.mean));
        }
    }
    *out = acc;
    *half_width = hw;
    *converged = conv;
    return eval_lp_result(lp_bad, acc, "evaluate_ci", pl.G);
}

extern "C" int twosd_evaluate_ci(twosd_ctx *c, const double *x, uint64_t seed, int64_t first, int64_t batch, int64_t n_max,
                                 double z, double rel_tol, double abs_tol, double offset, twosd_moments *out,
                                 double *half_width, int *converged) {
    return evaluate_ci(c, x, seed, first, batch, n_max, z, rel_tol, abs_tol, offset, out, half_width, converged, EvalPlan());
}

// the rule of twosd_evaluate_ci on the group moments: its scenario counts (done, n_max, batch) stay
// in scenarios, acc.n / acc.n_bad are groups
extern "C" int twosd_evaluate_ci_vr(twosd_ctx *c, const double *x, uint64_t seed, int64_t first, int64_t batch, int64_t n_max,
                                    double z, double rel_tol, double abs_tol, double offset, twosd_moments *out,
                                    double *half_width, int *converged, const twosd_sampling *plan) {
    EvalPlan pl;
    if (int rc = eval_plan(plan, "evaluate_ci", first, batch, "batch", &pl)) return rc;
    if (pl.G > 1) {
        if (batch / pl.G < 2)
            return fail(TWOSD_E_ARG, "evaluate_ci: batch = %lld holds fewer than 2 groups of %d", (long long)batch, pl.G);
        n_max = n_max / pl.G * pl.G;
    }
    return evaluate_ci(c, x, seed, first, batch, n_max, z, rel_tol, abs_tol, offset, out, half_width, converged, pl);
}

// Out-of-sample CVaR (risk.hip): the i.i.d. stream solved in evaluate_moments' chunks, every
// objective and status kept on the device (12 bytes per scenario), the level-quantile selected
// with unit weights, Y = var + max(obj - var, 0) / (1 - level) formed in place and reduced once
// over the whole range by the moments kernel.
extern "C" int twosd_evaluate_cvar(twosd_ctx *c, const double *x, uint64_t seed, int64_t first, int64_t count, double level,
                                   twosd_cvar *out) {
    int rc = eval_check_state(c, "evaluate_cvar");
    if (rc) return rc;
    if (!out || first < 0 || count < 1 || (c->n1 > 0 && !x)) return fail(TWOSD_E_ARG, "evaluate_cvar: bad arguments");
    if (!(level > 0.0 && level < 1.0)) return fail(TWOSD_E_ARG, "evaluate_cvar: level = %g outside (0, 1)", level);
    if (count > (1ll << 27))
        return fail(TWOSD_E_UNSUPPORTED, "evaluate_cvar: count = %lld scenarios exceed 2^27 (their objectives stay on the device)",
                    (long long)count);
    HIPCHK(hipSetDevice(c->device));
    RiskState &S = c->risk;
    if ((rc = S.obj.fit((size_t)count)) || (rc = S.ost.fit((size_t)count))) return rc;
    const int64_t chunk = eval_chunk_size(1);
    bool lp_bad = false;
    for (int64_t at = 0; at < count; at += chunk) {
        const int n = (int)std::min(chunk, count - at);
        rc = eval_solve_chunk(c, x, first + at, n, seed, EvalPlan());
        if (rc == TWOSD_E_LP) lp_bad = true;
        else if (rc) return rc;
        HIPCHK(hipMemcpyAsync(S.obj + at, c->d_obj, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(S.ost + at, c->d_status, sizeof(int) * n, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));   // the next solve may reallocate d_obj / d_status
    }
    *out = twosd_cvar{0, count, NAN, NAN, kMomentsEmpty};
    out->y.n_bad = count;
    RiskResult R{};
    if ((rc = risk_select(c, count, S.obj, nullptr, S.ost, 1.0, false, 0.0, level, "evaluate_cvar", &R)))
        return lp_bad && R.n_ok == 0 ? fail(TWOSD_E_LP, "evaluate_cvar: none of %lld scenario LPs is optimal", (long long)count) : rc;
    if ((rc = risk_form_y(c, count, S.obj, S.ost, R.var, 1.0 - level))) return rc;
    twosd_moments y;
    if ((rc = device_moments(c, count, S.obj, S.ost, nullptr, nullptr, &y))) return rc;
    out->n = y.n; out->n_bad = y.n_bad; out->var = R.var; out->cvar = y.mean; out->y = y;
    return eval_lp_result(lp_bad, y, "evaluate_cvar");
}

// evaluate(sp1, sp2, sto, x; N) stage-2 part (smps_routines.jl:67-82) on device-drawn
// scenarios: *s2 = sum over scenarios first..first+count-1 of the stream `seed`, in index
// order, of (1/N_total) * obj (s2_cost += 1/N*obj, :79).  Chunks of <= 1M scenarios (fixed: not
// TWOSD_EVAL_CHUNK), each drawn i.i.d. and solved by eval_solve_chunk, objectives summed on the
// host in order.
extern "C" int twosd_evaluate_sampled(twosd_ctx *c, const double *x, int64_t N_total, int64_t first, int64_t count,
                                      uint64_t seed, double *s2) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "evaluate_sampled: no template");
    if (!c->bp.has_basis) return fail(TWOSD_E_STATE, "evaluate_sampled: no warm-start basis");
    if (!c->has_dist) return fail(TWOSD_E_STATE, "evaluate_sampled: no distributions (twosd_set_distributions)");
    if (!s2 || N_total <= 0 || first < 0 || count < 0 || (c->n1 > 0 && !x)) return fail(TWOSD_E_ARG, "evaluate_sampled: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    const int64_t chunk = 1 << 20;
    const double invN = 1.0 / (double)N_total;
    double acc = 0.0;
    std::vector<double> obj;
    for (int64_t at = 0; at < count; at += chunk) {
        const int n = (int)std::min(chunk, count - at);
        obj.resize(n);
        if (int rc = eval_solve_chunk(c, x, first + at, n, seed, EvalPlan(), obj.data())) return rc;
        for (int i = 0; i < n; ++i) acc += invN * obj[i];
    }
    *s2 = acc;
    return TWOSD_OK;
}
