// lp_batch.hip -- one batch of scenario LPs: the launch (run_lp), the batch's reductions and copies
// to the host (copy_lp_outputs), the record of the last batch (twosd_ctx::last) with its getters,
// and the entry points that solve a batch (twosd_solve_batch / _values / _push).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "twosd_internal.h"
#include "twosd_ctx.h"

using namespace twosd;

// Launch the LP kernel over N scenarios whose deltas start at d_dv (device); results in
// c->d_obj / d_pi / d_y / d_status / d_iters [0, N).
// N = scenarios of d_dv addressed by the launch (outputs obj / status / iters / pool picks are
// indexed by scenario); list mode solves only o.d_list[0, o.nlist) from their recorded picks
// and writes pi at the list position
int twosd::run_lp(twosd_ctx *c, const double *x, const double *d_dv, int N, const LpRun &o) {
    const bool want_pi = o.want_pi, want_y = o.want_y;
    const bool list = o.d_list != nullptr;
    const int NL = list ? o.nlist : N;   // scenarios this launch solves
    int rc;
    if (o.want_ray && !list) return fail(TWOSD_E_ARG, "LP rays: list mode only");
    if ((rc = prepare_x(c, x))) return rc;
    if (list &&c->bp.bases.size() > 1 && (size_t)N > c->d_pool_pick.cap) return fail(TWOSD_E_STATE, "LP list mode: no recorded pool picks");
    const int m = c->L.m, n = c->L.n, MP = c->MP, R = c->R;
    if (N > c->out_cap) {
        size_t cap = std::max<size_t>(N, 1024);
        if ((rc = c->d_obj.alloc(cap)) || (rc = c->d_status.alloc(cap)) || (rc = c->d_iters.alloc(cap)) ||
            (rc = c->d_ops.alloc(cap)) || (rc = c->d_etan.alloc(cap)))
            return rc;
        c->d_pi.release(); c->d_y.release();
        c->out_cap = (int)cap;
    }
    // the optional outputs, out_cap rows each, on their first use at this out_cap
    if (want_pi && (size_t)NL * m > c->d_pi.cap && (rc = c->d_pi.alloc((size_t)c->out_cap * m))) return rc;
    if (o.want_key && (size_t)N > c->d_vkey.cap && (rc = c->d_vkey.alloc((size_t)c->out_cap))) return rc;
    if (o.want_bkey && (size_t)N > c->d_bkey.cap && (rc = c->d_bkey.alloc((size_t)c->out_cap))) return rc;
    if (want_y && (size_t)N * n > c->d_y.cap && (rc = c->d_y.alloc((size_t)c->out_cap * n))) return rc;
    if (!c->d_queue && (rc = c->d_queue.alloc((size_t)kMaxQueueGroups * kQueueStride))) return rc;
    {
        // eta capacity (pivots per scenario): 2m + 32, at least 64.  256 keeps storm's two 4-wave
        // blocks per CU within the LDS; past 256 the file grows (up to 1024, in steps of 32) as far as
        // the LDS keeps the occupancy of 256 -- a scenario that needs more pivots from its pool start
        // than the file holds is retried from the primary basis (ssn 100k: 11 in 8 steps at 256)
        const int CH = c->CH;
        int kmax = c->kmax_override > 0 ? c->kmax_override : std::min(256, std::max(64, 2 * m + 32));
        if (c->kmax_override <= 0 && 2 * m + 32 > kmax) {
            const int b0 = hyper_max_blocks_per_cu(R, CH, kmax, c->k);
            for (int k2 = std::min(1024, (2 * m + 32) & ~31); k2 > kmax; k2 -= 32)
                if (hyper_max_blocks_per_cu(R, CH, k2, c->k) >= b0) { kmax = k2; break; }
        }
        // per-wave eta arena: 32 entries per row, scaled with the file past 256 pivots
        const int ecap = (int)std::min<long long>(INT32_MAX / 2, (long long)std::max(4096, 32 * MP) * std::max(256, kmax) / 256);
        int bpc = hyper_max_blocks_per_cu(R, CH, kmax, c->k);
        if (const char *e = getenv("TWOSD_BPC")) bpc = std::min(bpc, std::max(1, atoi(e)));   // diagnostics: occupancy sweep
        if (bpc < 1)
            return fail(TWOSD_E_UNSUPPORTED, "LP kernel: LDS slice too large (m2 = %d, n2 = %d; LP: %d rows, %d columns; k = %d)",
                        c->m2_user, c->n2_user, m, n, c->k);
        const int nblocks = std::max(1, std::min((NL + kWavesPerBlock - 1) / kWavesPerBlock, bpc * c->num_cus));
        const size_t slots = (size_t)nblocks * kWavesPerBlock;
        if (slots > c->earena_slots || ecap != c->earena_cap) {
            if ((rc = c->d_eidx.alloc(slots * ecap)) || (rc = c->d_evals.alloc(slots * ecap))) return rc;
            c->earena_slots = slots;
            c->earena_cap = ecap;
        }
        HIPCHK(hipMemsetAsync(c->d_queue, 0, sizeof(int) * kMaxQueueGroups * kQueueStride, c->stream));
        HyperParams H{};
        H.m = m; H.n = n; H.k = c->k; H.N = NL; H.kmax = kmax; H.ecap = ecap;
        H.kcap = o.kcap > 0 ? std::min(o.kcap, kmax) : kmax;
        H.retry = o.kcap > 0 ? 0 : 1;
        H.colptr = c->d_colptr; H.rowidx = c->d_rowidx; H.val = c->d_val; H.q = c->d_q; H.btype = c->d_btype;
        H.wcp = c->d_wcp; H.wcc = c->d_wcc; H.wcv = c->d_wcv;
        const PoolArrays pa = pool_arrays(c);
        H.bcp = pa.bcp; H.bci = pa.bci; H.bcv = pa.bcv;
        H.brptr = pa.brptr; H.brcol = pa.brcol; H.brval = pa.brval;
        H.kslot = pa.kslot; H.kix = pa.kix; H.kv = pa.kv; H.kcoef = c->d_kcoef;
        H.xbase = c->d_xbase; H.d0 = pa.d0; H.hb0 = pa.hb0;
        H.basic0 = pa.basic0; H.fixedmask = c->d_fixedmask; H.ubmask = c->d_ubmask;
        H.dv = d_dv; H.eidx = c->d_eidx; H.evals = c->d_evals; H.queue = c->d_queue;
        H.qgroups = std::max(1, std::min(16, nblocks));   // two ranges per XCD (8 / 16 / 32 / 64: 143.6 / 142.7 / 142.8 / 146.3 ms, storm 1M)
        if (const char *e = getenv("TWOSD_QGROUPS")) H.qgroups = std::max(1, std::min({kMaxQueueGroups, nblocks, atoi(e)}));   // A/B knob
        H.obj = c->d_obj; H.pi = want_pi ? c->d_pi : nullptr; H.y = want_y ? c->d_y : nullptr;
        H.vkey = o.want_key ? c->d_vkey : nullptr;
        H.key_zero = 1e-12;   // = HPI_ZERO of the pi recovery (lp_hyper.hip)
        if (const char *e = getenv("TWOSD_KEY_ZERO")) H.key_zero = atof(e);   // A/B knob
        H.bkey = o.want_bkey ? c->d_bkey : nullptr;
        if (o.want_etas) {   // rows: list positions, or scenarios
            const size_t need = list ? (size_t)NL : (size_t)N;
            // eta-file offsets are 32-bit (eo_off, the device pool build): the arena of
            // 4096 entries per row must stay below 2^31 entries
            if (need * 4096 > (size_t)INT32_MAX)
                return fail(TWOSD_E_UNSUPPORTED, "eta files of %zu solves exceed the 2^31-entry arena (at most %d)", need,
                            INT32_MAX / 4096);
            // the arena: 4096 entries per row, or what an earlier training run asked for
            // (refresh_training solves again when the eta files did not fit)
            const size_t cap_need = std::max(std::max<size_t>(need, 256) * 4096, c->eo_min_cap);
            if (need > c->eo_rows || c->eo_kmax != kmax || c->eo_cap < cap_need) {
                const size_t rows = std::max<size_t>(need, 256);
                if ((rc = c->d_eo_pb.alloc(rows)) || (rc = c->d_eo_K.alloc(rows)) || (rc = c->d_eo_off.alloc(rows)) ||
                    (rc = c->d_eo_etap.alloc(rows * kmax)) || (rc = c->d_eo_etaoff.alloc(rows * (kmax + 1))) ||
                    (rc = c->d_eo_eidx.alloc(cap_need)) || (rc = c->d_eo_evals.alloc(cap_need)))
                    return rc;
                if (!c->d_eo_used && (rc = c->d_eo_used.alloc(1))) return rc;
                c->eo_rows = rows;
                c->eo_cap = cap_need;
                c->eo_kmax = kmax;
            }
            HIPCHK(hipMemsetAsync(c->d_eo_used, 0, sizeof(unsigned long long), c->stream));
            H.eo_pb = c->d_eo_pb; H.eo_K = c->d_eo_K; H.eo_off = c->d_eo_off; H.eo_etap = c->d_eo_etap;
            H.eo_etaoff = c->d_eo_etaoff; H.eo_eidx = c->d_eo_eidx; H.eo_evals = c->d_eo_evals; H.eo_used = c->d_eo_used;
            H.eo_cap = (long long)std::min<size_t>(c->eo_cap, INT32_MAX);
        }
        if (o.want_head) {   // rows: list positions, or scenarios
            const size_t need = list ? (size_t)NL : (size_t)N;
            if ((rc = c->d_head_out.fit(need * m))) return rc;
            H.head_out = c->d_head_out;
        }
        if (o.want_ray) {   // rows: list positions; a position that does not end infeasible keeps row -1 and key 0
            FrayState &Fs = c->fray;
            if ((rc = Fs.ray.fit((size_t)NL * m)) || (rc = Fs.ray_row.fit((size_t)NL)) || (rc = Fs.ray_key.fit((size_t)NL))) return rc;
            HIPCHK(hipMemsetAsync(Fs.ray_row, 0xff, sizeof(int) * NL, c->stream));
            HIPCHK(hipMemsetAsync(Fs.ray_key, 0, sizeof(unsigned long long) * NL, c->stream));
            H.ray = Fs.ray; H.ray_row = Fs.ray_row; H.ray_key = Fs.ray_key;
        }
        H.pi_by_pos = list ? 1 : 0;
        H.status = c->d_status; H.iters = c->d_iters; H.ops = c->d_ops; H.etan = c->d_etan;
        if (!c->d_lpstats && (rc = c->d_lpstats.alloc(6))) return rc;
        if (!list) HIPCHK(hipMemsetAsync(c->d_lpstats + 5, 0, sizeof(unsigned long long), c->stream));
        H.retries = list ? nullptr : c->d_lpstats + 5;   // a list re-solve repeats recorded picks: no retries
        if (!c->d_stamps) {
            if ((rc = c->d_stamps.alloc(16))) return rc;
            HIPCHK(hipMemset(c->d_stamps, 0, sizeof(unsigned long long) * 16));
        }
        H.stamps = c->d_stamps;
        H.npool = (int)c->bp.bases.size();
        H.bnnz = pa.bnnz;
        if (H.npool > 1) {
            if (!list && (rc = c->d_pool_pick.fit((size_t)N))) return rc;
            H.pool_pick = c->d_pool_pick;
        }
        if (!list && pa.kslot && getenv("TWOSD_DEBUG")) {
            // w, the widest ELL slot of a start basis: the x_B warm start walks w columns
            std::vector<int> ks((size_t)H.npool * (R + 1));
            HIPCHK(hipMemcpy(ks.data(), pa.kslot, sizeof(int) * ks.size(), hipMemcpyDeviceToHost));
            std::vector<int> ws(H.npool);
            double mean = 0;
            for (int p = 0; p < H.npool; ++p) {
                int w = 0;
                for (int t = 0; t < R; ++t) w = std::max(w, ks[(size_t)p * (R + 1) + t + 1] - ks[(size_t)p * (R + 1) + t]);
                ws[p] = w;
                mean += w;
            }
            std::sort(ws.begin(), ws.end());
            fprintf(stderr, "LP start: ELL width w over %d bases: min %d, median %d, mean %.2f, p90 %d, max %d\n", H.npool, ws.front(),
                    ws[ws.size() / 2], mean / H.npool, ws[ws.size() * 9 / 10], ws.back());
        }
        HIPCHK(hipEventRecord(c->ev[EV_LP_BEGIN], c->stream));
        const int *order = nullptr;
        if (list) {
            order = o.d_list;
        } else if (H.npool > 1) {
            if ((rc = select_pool(c, d_dv, N, c->d_pool_pick, 0))) return rc;
            order = c->d_order;
        }
        HIPCHK(hipEventRecord(c->ev[EV_LP_SELECTED], c->stream));
        // one record per queue position (its scenario and start basis), so that a wave learns both
        // from its claim in one load; part of the timed LP launch.  Neither an order nor a pool:
        // position q is scenario q from the primary basis and the kernel reads no record.
        if (order || H.npool > 1) {
            if ((rc = c->d_qrec.fit(std::max<size_t>(NL, 1024)))) return rc;
            HIPCHK(launch_queue_records(order, H.npool > 1 ? c->d_pool_pick : nullptr, c->d_qrec, NL, c->stream));
            H.qrec = c->d_qrec;
        }
        HIPCHK(launch_hyper(R, CH, H, nblocks, hyper_lds_bytes(R, CH, kmax, c->k), c->stream));
        HIPCHK(hipEventRecord(c->ev[EV_LP_END], c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        float ms = 0, ms_sel = 0;
        hipEventElapsedTime(&ms, c->ev[EV_LP_SELECTED], c->ev[EV_LP_END]);
        hipEventElapsedTime(&ms_sel, c->ev[EV_LP_BEGIN], c->ev[EV_LP_SELECTED]);
        if (list) {   // the record stays the main batch's (LpBatchRecord)
            if (o.lp_us_out) *o.lp_us_out = 1e3 * ms;
            return TWOSD_OK;
        }
        c->last.N = N;
        c->last.lp_us = 1e3 * ms;
        c->last.sel_us = 1e3 * ms_sel;
        return TWOSD_OK;
    }
}

// batch statistics on the device (integer sums: exact, order independent): [0] pivots,
// [1] executed FMAs, [2] max pivots, [3] non-optimal scenarios
__global__ void __launch_bounds__(256) lp_stats_kernel(int N, const int *__restrict__ its, const long long *__restrict__ ops,
                                                      const int *__restrict__ st, const int *__restrict__ etan,
                                                      unsigned long long *out) {
    __shared__ unsigned long long red[4][5];
    unsigned long long a = 0, b = 0, d = 0, e = 0;
    unsigned long long mx = 0;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < N; s += gridDim.x * blockDim.x) {
        a += (unsigned long long)its[s];
        b += (unsigned long long)ops[s];
        mx = its[s] > (int)mx ? (unsigned long long)its[s] : mx;
        d += st[s] != TWOSD_LP_OPTIMAL;
        e += (unsigned long long)etan[s];
    }
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o);
        b += __shfl_down(b, o);
        d += __shfl_down(d, o);
        e += __shfl_down(e, o);
        const unsigned long long m2 = __shfl_down(mx, o);
        mx = m2 > mx ? m2 : mx;
    }
    // one set of atomics per block (per wave they serialised on five addresses: ~0.25 ms at 1M)
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[w][0] = a; red[w][1] = b; red[w][2] = mx; red[w][3] = d; red[w][4] = e;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < (int)(blockDim.x >> 6); ++v) {
            a += red[v][0]; b += red[v][1]; mx = red[v][2] > mx ? red[v][2] : mx; d += red[v][3]; e += red[v][4];
        }
        atomicAdd(&out[0], a);
        atomicAdd(&out[1], b);
        atomicMax(&out[2], mx);
        atomicAdd(&out[3], d);
        atomicAdd(&out[4], e);
    }
}

// incumbent objective of a batch: sum_s w_s obj_s and sum_s w_s (w = 1 without weights), each
// block over a fixed stride of scenarios, then a fixed tree in the block; the host adds the
// kObjBlocks partials in block order, so the sums do not depend on scheduling
constexpr int kObjBlocks = 256;
__global__ void __launch_bounds__(256) lp_obj_kernel(int N, const double *__restrict__ obj, const double *__restrict__ w,
                                                     double *__restrict__ part) {
    __shared__ double sa[256], sb[256];
    double a = 0.0, b = 0.0;
    for (int s = blockIdx.x * 256 + threadIdx.x; s < N; s += kObjBlocks * 256) {
        const double ws = w ? w[s] : 1.0;
        a = fma(ws, obj[s], a);
        b += ws;
    }
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sa[threadIdx.x] += sa[threadIdx.x + o];
            sb[threadIdx.x] += sb[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sa[0];
        part[2 * blockIdx.x + 1] = sb[0];
    }
}

// Template with general bounds: the LP's outputs back into the caller's space.  yu[s][j] =
// off[j] + sign[j] * y[s][src[j]] - y[s][src2[j]] (a term with index -1 is absent: fixed columns
// have no LP column, only free ones a second), one thread per output entry, j fastest, so a wave
// writes consecutive entries of a row and reads a (nearly) consecutive run of the LP's row; and
// obj[s] += c0, the constant q.s the shift took out of the LP.  y / yu nullable (objectives only).
__global__ void __launch_bounds__(256) bounds_backmap_kernel(int N, int n2, int n_lp, const int *__restrict__ src,
                                                             const int *__restrict__ src2, const double *__restrict__ sign,
                                                             const double *__restrict__ off, const double *__restrict__ y,
                                                             double *__restrict__ yu, double c0, double *__restrict__ obj) {
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    for (size_t s = t0; s < (size_t)N; s += step) obj[s] += c0;
    if (!y) return;
    const size_t tot = (size_t)N * n2;
    for (size_t i = t0; i < tot; i += step) {
        const size_t s = i / n2;
        const int j = (int)(i - s * n2);
        const double *row = y + s * n_lp;
        const int a = src[j], b = src2[j];
        double v = off[j];
        if (a >= 0) v = fma(sign[j], row[a], v);
        if (b >= 0) v -= row[b];
        yu[i] = v;
    }
}

// d_w: the batch's scenario weights (nullable: 1.0), for the objective sum
int twosd::copy_lp_outputs(twosd_ctx *c, int N, double *obj, double *pi, double *y, int *status, const double *d_w) {
    if (!c->d_lpstats) {
        int rc = c->d_lpstats.alloc(6);
        if (rc) return rc;
    }
    if (!c->d_objpart) {
        int rc = c->d_objpart.alloc((size_t)2 * kObjBlocks);
        if (rc) return rc;
    }
    const double *d_yout = c->d_y;
    if (c->has_bounds) {   // before the objective sum and the copies: they see the caller's values
        if (y && (size_t)N * c->n2_user > c->d_yu.cap) {
            int rc = c->d_yu.alloc((size_t)std::max(N, c->out_cap) * c->n2_user);
            if (rc) return rc;
        }
        const size_t work = y ? (size_t)N * c->n2_user : (size_t)N;
        hipLaunchKernelGGL(bounds_backmap_kernel, dim3((unsigned)std::min<size_t>(4096, (work + 255) / 256)), dim3(256), 0, c->stream, N,
                           c->n2_user, c->L.n, c->d_bm_src, c->d_bm_src2, c->d_bm_sign, c->d_bm_off, y ? c->d_y : nullptr,
                           y ? c->d_yu : nullptr, c->c0, c->d_obj);
        HIPCHK(hipGetLastError());
        d_yout = c->d_yu;
    }
    HIPCHK(hipMemsetAsync(c->d_lpstats, 0, 5 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(lp_stats_kernel, dim3((unsigned)std::min(256, (N + 255) / 256)), dim3(256), 0, c->stream, N,
                       c->d_iters, c->d_ops, c->d_status, c->d_etan, c->d_lpstats);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(lp_obj_kernel, dim3(kObjBlocks), dim3(256), 0, c->stream, N, c->d_obj, d_w, c->d_objpart);
    HIPCHK(hipGetLastError());
    unsigned long long stv[6];
    double part[2 * kObjBlocks];
    HIPCHK(hipMemcpyAsync(stv, c->d_lpstats, sizeof(stv), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(part, c->d_objpart, sizeof(part), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (obj) HIPCHK(hipMemcpy(obj, c->d_obj, sizeof(double) * N, hipMemcpyDeviceToHost));
    if (pi) HIPCHK(hipMemcpy(pi, c->d_pi, sizeof(double) * N * c->L.m, hipMemcpyDeviceToHost));
    if (y) HIPCHK(hipMemcpy(y, d_yout, sizeof(double) * N * c->n2_user, hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, c->d_status, sizeof(int) * N, hipMemcpyDeviceToHost));
    LpBatchRecord &L = c->last;
    L.pivots_sum = (int64_t)stv[0]; L.ops_sum = (int64_t)stv[1]; L.pivots_max = (int)stv[2];
    L.eta_entries = (int64_t)stv[4];
    L.retries = (int64_t)stv[5];
    if (N >= 4096) {
        c->piv_ref_sum = (int64_t)stv[0];
        c->piv_ref_n = N;
    }
    double ow = 0.0, wt = 0.0;
    for (int b = 0; b < kObjBlocks; ++b) {
        ow += part[2 * b];
        wt += part[2 * b + 1];
    }
    L.obj_wsum = ow;
    L.obj_w = wt;
    const long long bad = (long long)stv[3];
    if (bad) return fail(TWOSD_E_LP, "%lld of %d scenario LPs not optimal (see status[])", bad, N);
    return TWOSD_OK;
}

extern "C" int twosd_last_objective(twosd_ctx *c, double *weighted_sum, double *weight_sum) {
    if (!c) return fail(TWOSD_E_ARG, "last_objective: NULL");
    if (weighted_sum) *weighted_sum = c->last.obj_wsum;
    if (weight_sum) *weight_sum = c->last.obj_w;
    return TWOSD_OK;
}

extern "C" int twosd_solve_batch(twosd_ctx *c, int epi, const double *x, int first, int count, double *obj,
                                 double *pi, double *y, int *status) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "solve_batch: no template");
    if (!c->bp.has_basis) return fail(TWOSD_E_STATE, "solve_batch: no warm-start basis (twosd_compute_basis / twosd_set_basis)");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "solve_batch: epigraph %d does not exist", epi);
    const EpiDevice &E = c->epis[epi];
    if (first < 0 || count < 0 || first + count > E.count) return fail(TWOSD_E_ARG, "solve_batch: range [%d,%d) outside %d scenarios", first, first + count, E.count);
    if (!obj || !status || (c->n1 > 0 && !x)) return fail(TWOSD_E_ARG, "solve_batch: obj/status/x required");
    if (count == 0) return TWOSD_OK;
    HIPCHK(hipSetDevice(c->device));
    LpRun o;
    o.want_pi = pi != nullptr;
    o.want_y = y != nullptr;
    int rc = run_lp(c, x, E.d_dv + (size_t)first * c->k, count, o);
    if (rc) return rc;
    return copy_lp_outputs(c, count, obj, pi, y, status, E.d_w + first);
}

extern "C" int twosd_solve_values(twosd_ctx *c, const double *x, int N, const double *values, double *obj, double *pi,
                                  double *y, int *status) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "solve_values: no template");
    if (!c->bp.has_basis) return fail(TWOSD_E_STATE, "solve_values: no warm-start basis");
    if (N < 0 || (N > 0 && c->k > 0 && !values) || !obj || !status || (c->n1 > 0 && !x)) return fail(TWOSD_E_ARG, "solve_values: bad arguments");
    if (N == 0) return TWOSD_OK;
    HIPCHK(hipSetDevice(c->device));
    const int k = c->k;
    std::vector<double> dv((size_t)N * std::max(k, 1), 0.0);
    for (int s = 0; s < N; ++s)
        for (int e = 0; e < k; ++e) dv[(size_t)s * k + e] = values[(size_t)s * k + e] - template_value(c, e);
    int rc;
    if ((rc = c->d_dvtmp.grow((size_t)N * std::max(k, 1), 0, c->stream))) return rc;
    HIPCHK(hipMemcpy(c->d_dvtmp, dv.data(), sizeof(double) * dv.size(), hipMemcpyHostToDevice));
    LpRun o;
    o.want_pi = pi != nullptr;
    o.want_y = y != nullptr;
    if ((rc = run_lp(c, x, c->d_dvtmp, N, o))) return rc;
    return copy_lp_outputs(c, N, obj, pi, y, status, nullptr);
}

extern "C" int twosd_last_timings(twosd_ctx *c, double *us5) {
    if (!c || !us5) return fail(TWOSD_E_ARG, "last_timings: NULL");
    for (int i = 0; i < T_COUNT; ++i) us5[i] = c->t_us[i];
    us5[T_LP] = c->last.lp_us;
    us5[T_POOL_SELECT] = c->last.sel_us;
    return TWOSD_OK;
}

extern "C" int twosd_last_lp_eta_entries(twosd_ctx *c, int64_t *entries, int64_t *retries) {
    if (!c || !entries) return fail(TWOSD_E_ARG, "last_lp_eta_entries: NULL");
    *entries = c->last.eta_entries;
    if (retries) *retries = c->last.retries;
    return TWOSD_OK;
}

extern "C" int twosd_last_lp_stats(twosd_ctx *c, int64_t *sum, int *mx) {
    if (!c) return fail(TWOSD_E_ARG, "last_lp_stats: NULL");
    if (sum) *sum = c->last.pivots_sum;
    if (mx) *mx = c->last.pivots_max;
    return TWOSD_OK;
}

extern "C" int twosd_last_lp_iters(twosd_ctx *c, int N, int *iters, int *status) {
    if (!c || N < 0 || N > c->out_cap || !c->d_iters) return fail(TWOSD_E_ARG, "last_lp_iters: N = %d outside the last batch", N);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (iters) HIPCHK(hipMemcpy(iters, c->d_iters, sizeof(int) * N, hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, c->d_status, sizeof(int) * N, hipMemcpyDeviceToHost));
    return TWOSD_OK;
}

extern "C" int twosd_debug_stamps(twosd_ctx *c, uint64_t *out10, int reset) {
    if (!c || !out10) return fail(TWOSD_E_ARG, "debug_stamps: NULL");
    for (int i = 0; i < 10; ++i) out10[i] = 0;
    if (!c->d_stamps) return TWOSD_OK;
    HIPCHK(hipMemcpy(out10, c->d_stamps, sizeof(uint64_t) * 10, hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(c->d_stamps, 0, sizeof(uint64_t) * 16));
    return TWOSD_OK;
}

extern "C" int twosd_last_lp_ops(twosd_ctx *c, int64_t *row_ops, int *row_width) {
    if (!c) return fail(TWOSD_E_ARG, "last_lp_ops: NULL");
    if (row_ops) *row_ops = c->last.ops_sum;
    if (row_width) *row_width = 1;   // the count is in FMAs
    return TWOSD_OK;
}

// rows list[0..U) of pi (m doubles each) gathered in list order (the push of a full-mode solve_push)
__global__ void gather_rows_kernel(int U, int m, const int *__restrict__ list, const double *__restrict__ pi, double *__restrict__ out) {
    const size_t tot = (size_t)U * m;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) {
        const int u = (int)(i / m), r = (int)(i % m);
        out[i] = pi[(size_t)list[u] * m + r];
    }
}

// non-optimal statuses among the scenarios of a list-mode re-solve (status is by scenario)
__global__ void list_status_kernel(int U, const int *__restrict__ list, const int *__restrict__ st,
                                   unsigned long long *bad) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < U; i += gridDim.x * blockDim.x)
        if (st[list[i]] != TWOSD_LP_OPTIMAL) atomicAdd(bad, 1ull);
}

extern "C" int twosd_solve_push(twosd_ctx *c, int epi, const double *x, int first, int count, double *obj, int *status,
                                int *new_size) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "solve_push: no template");
    if (!c->bp.has_basis) return fail(TWOSD_E_STATE, "solve_push: no warm-start basis");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "solve_push: epigraph %d does not exist", epi);
    const EpiDevice &E = c->epis[epi];
    if (first < 0 || count < 0 || first + count > E.count) return fail(TWOSD_E_ARG, "solve_push: range outside the epigraph");
    if (c->n1 > 0 && !x) return fail(TWOSD_E_ARG, "solve_push: x is NULL");
    if (count == 0) { if (new_size) *new_size = c->dvs.size; return TWOSD_OK; }
    HIPCHK(hipSetDevice(c->device));
    const double *d_dv = E.d_dv + (size_t)first * c->k;
    // TWOSD_PUSH_ALL=1: recover and push the dual of every scenario (the pre-key path, kept for
    // the equivalence test); default: vertex keys, first occurrences, re-solve of those only
    const bool all = getenv("TWOSD_PUSH_ALL") && atoi(getenv("TWOSD_PUSH_ALL")) != 0;
    // Full mode: the main pass recovers every scenario's dual (and its key), and the representatives'
    // rows are gathered from it -- the same rows the re-solve would produce (same start, same pivots,
    // same recovery), without solving them twice.  Chosen when the last keyed push re-solved more
    // than a quarter of its scenarios (ssn: ~every scenario its own vertex; storm: < 1 %).
    // TWOSD_PUSH_MODE: 0 auto (default), 1 always re-solve, 2 always full.
    const int pmode = getenv("TWOSD_PUSH_MODE") ? atoi(getenv("TWOSD_PUSH_MODE")) : 0;
    const bool full = !all && (pmode == 2 || (pmode == 0 && c->push_rep_frac > 0.25));
    c->last_push_full = full ? 1 : 0;
    LpRun o;
    o.want_pi = all || full;
    o.want_key = !all;
    int rc = run_lp(c, x, d_dv, count, o);
    if (rc) return rc;
    rc = copy_lp_outputs(c, count, obj, nullptr, nullptr, status, E.d_w + first);
    if (rc) return rc;   // some LP not optimal: nothing pushed
    // c->last is now the batch's and stays it: the representatives' re-solve below is a list-mode
    // launch, which only hands back its kernel time
    float ms = 0, ms_key = 0;
    const auto timed_push = [c](int n, const double *d_rows, float *ms_out) -> int {
        HIPCHK(hipEventRecord(c->ev[EV_PUSH_BEGIN], c->stream));
        if (int r = dvs_push_device(c, n, d_rows, nullptr)) return r;
        HIPCHK(hipEventRecord(c->ev[EV_PUSH_END], c->stream));
        HIPCHK(hipEventSynchronize(c->ev[EV_PUSH_END]));
        hipEventElapsedTime(ms_out, c->ev[EV_PUSH_BEGIN], c->ev[EV_PUSH_END]);
        return TWOSD_OK;
    };
    if (all) {
        if ((rc = timed_push(count, c->d_pi, &ms))) return rc;
        c->last_push_reps = count;
    } else {
        HIPCHK(hipEventRecord(c->ev[EV_MARK_1], c->stream));
        const int *d_list = nullptr;
        int U = 0;
        if ((rc = vkey_first_occurrences(c, count, c->d_vkey, c->d_status, &d_list, &U))) return rc;
        HIPCHK(hipEventRecord(c->ev[EV_MARK_2], c->stream));
        HIPCHK(hipEventSynchronize(c->ev[EV_MARK_2]));
        hipEventElapsedTime(&ms_key, c->ev[EV_MARK_1], c->ev[EV_MARK_2]);
        c->last_push_reps = U;
        c->push_rep_frac = (double)U / count;
        if (U > 0 && full) {
            const int m = c->L.m;
            if ((rc = c->d_pi_rep.fit((size_t)U * m))) return rc;
            hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)std::min<size_t>(4096, ((size_t)U * m + 255) / 256)), dim3(256), 0,
                               c->stream, U, m, d_list, c->d_pi, c->d_pi_rep);
            HIPCHK(hipGetLastError());
            if ((rc = timed_push(U, c->d_pi_rep, &ms))) return rc;
        } else if (U > 0) {
            double resolve_us = 0.0;
            LpRun r;
            r.want_pi = true;
            r.d_list = d_list;
            r.nlist = U;
            r.lp_us_out = &resolve_us;
            if ((rc = run_lp(c, x, d_dv, count, r))) return rc;
            // the re-solve starts every representative from its recorded pick and repeats its
            // optimal solve; should one ever end otherwise, its pi row must not reach V
            HIPCHK(hipMemsetAsync(c->d_lpstats, 0, sizeof(unsigned long long), c->stream));
            hipLaunchKernelGGL(list_status_kernel, dim3((unsigned)std::min(256, (U + 255) / 256)), dim3(256), 0, c->stream, U,
                               d_list, c->d_status, c->d_lpstats);
            HIPCHK(hipGetLastError());
            unsigned long long bad = 0;
            HIPCHK(hipMemcpyAsync(&bad, c->d_lpstats, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            if (bad) return fail(TWOSD_E_LP, "solve_push: %llu of %d re-solved representatives not optimal; nothing pushed", bad, U);
            c->last.lp_us += resolve_us;   // LP kernel time of the batch: main pass + representatives
            if ((rc = timed_push(U, c->d_pi, &ms))) return rc;
        }
    }
    c->t_us[T_DEDUP] = 1e3 * (ms + ms_key);
    if (new_size) *new_size = c->dvs.size;
    return TWOSD_OK;
}

extern "C" int twosd_last_push_mode(twosd_ctx *c, int *full) {
    if (!c || !full) return fail(TWOSD_E_ARG, "last_push_mode: NULL");
    *full = c->last_push_full;
    return TWOSD_OK;
}

extern "C" int twosd_last_push_reps(twosd_ctx *c, int *reps) {
    if (!c || !reps) return fail(TWOSD_E_ARG, "last_push_reps: NULL");
    *reps = c->last_push_reps;
    return TWOSD_OK;
}
