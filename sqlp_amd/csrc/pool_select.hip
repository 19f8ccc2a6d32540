// pool_select.hip -- warm-start selection from the basis pool: the x-independent element rows of
// the pool (prepare_elements), the per-x preparation (prepare_x: x_B of every basis and the
// selection stream), the flat and two-level selection of a batch (select_pool) and the candidate
// lists of the two-level form.  The pool itself (host forms, device arrays, upload, validity) is
// basis_pool.hip's; this file reads it through pool_host_rows and pool_arrays.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <chrono>
#include "twosd_internal.h"
#include "twosd_ctx.h"

using namespace twosd;

// the two-level candidate lists (device, or staged for the next selection) refer to pool
// indices: every change of the pool drops them
void twosd::reset_candidates(twosd_ctx *c) {
    c->pool_l1 = c->pool_ncand = 0;
    c->cand_pending = false;
    std::vector<int>().swap(c->cand_p1);
    std::vector<int>().swap(c->cand_pf);
}

// device selection-stream outputs of a pool of P bases with `records` records (prepare_x
// writes them per x)
int twosd::reserve_selection(twosd_ctx *c, int P, int records) {
    int rc;
    if ((rc = c->d_sel_code.fit(2 * (size_t)std::max(records, 1)))) return rc;   // (code, float bits) pairs
    if ((rc = c->d_sel_end.reserve((size_t)P)) || (rc = c->d_sel_cinf.reserve((size_t)P))) return rc;
    c->sel_cap_total = records;
    return TWOSD_OK;
}

int twosd::training_box(twosd_ctx *c, const EpiDevice &E, int epi, int first, int count, std::vector<double> &lo,
                        std::vector<double> &hi, BoxCache *cache) {
    const int k = c->k;
    const BoxCache range{epi, first, count, E.count};
    if (k <= 0 || (cache && *cache == range)) return TWOSD_OK;
    std::vector<double> dv((size_t)count * k);
    HIPCHK(hipMemcpy(dv.data(), E.d_dv + (size_t)first * k, sizeof(double) * dv.size(), hipMemcpyDeviceToHost));
    lo.assign(k, INFINITY);
    hi.assign(k, -INFINITY);
    for (int s = 0; s < count; ++s)
        for (int e = 0; e < k; ++e) {
            lo[e] = std::min(lo[e], dv[(size_t)s * k + e]);
            hi[e] = std::max(hi[e], dv[(size_t)s * k + e]);
        }
    if (cache) *cache = range;
    return TWOSD_OK;
}

// x-independent element data of the pool (rebuilt when the pool or the positions change):
// per basis p the rows of B_p^{-1}[:, row_e] over the random elements e (host CSR kptr/ke/
// kraw, e ascending) and the same as sliced ELL on the device (kslot pool-strided, absolute
// into kix/kv).  The kernels multiply the scenario deltas by coef_e(x) (d_kcoef) themselves.
int twosd::prepare_elements(twosd_ctx *c) {
    const auto t_pe0 = std::chrono::steady_clock::now();
    if (int rc0 = pool_host_rows(c)) return rc0;
    const int m = c->L.m, k = c->k, R = c->R;
    std::vector<std::vector<int>> bycol(m);   // random elements on each row
    for (int e = 0; e < k; ++e) bycol[c->pos_row[e]].push_back(e);
    const int P = (int)c->bp.bases.size();
    std::vector<int8_t> bt(c->L.n + m);
    HIPCHK(hipMemcpy(bt.data(), c->d_btype, bt.size(), hipMemcpyDeviceToHost));
    // pass 1: per basis and row the number of element entries; CSR / ELL / record sizes
    std::vector<int> rowcnt((size_t)P * m), width((size_t)P * R);
    std::vector<size_t> kcnt(P + 1, 0), ecnt(P + 1, 0);
    std::vector<int64_t> ccnt(P + 1, 0);
    parallel_for(P, [&](int p) {
        const PoolBasis &B = c->bp.bases[p];
        int *rc = rowcnt.data() + (size_t)p * m;
        size_t tot = 0;
        int64_t cp = 0;   // selection records: every row active; rows of fixed (E) basics twice
        for (int i = 0; i < m; ++i) {
            int n_i = 0;
            for (int q = B.rptr[i]; q < B.rptr[i + 1]; ++q) n_i += (int)bycol[B.rcol[q]].size();
            rc[i] = n_i;
            tot += n_i;
            cp += (int64_t)(1 + n_i) * (bt[B.head[i]] == BT_E ? 2 : 1);
        }
        size_t ell = 0;
        for (int t = 0; t < R; ++t) {
            int w = 0;
            for (int l = 0; l < 64 && 64 * t + l < m; ++l) w = std::max(w, rc[64 * t + l]);
            width[(size_t)p * R + t] = w;
            ell += (size_t)w * 64;
        }
        kcnt[p + 1] = tot;
        ecnt[p + 1] = ell;
        ccnt[p + 1] = cp;
    });
    for (int p = 0; p < P; ++p) { kcnt[p + 1] += kcnt[p]; ecnt[p + 1] += ecnt[p]; ccnt[p + 1] += ccnt[p]; }
    if (kcnt[P] > INT32_MAX || ecnt[P] / 64 > INT32_MAX || ccnt[P] > INT32_MAX)
        return fail(TWOSD_E_UNSUPPORTED, "basis pool element data too large (> 2^31 entries)");
    // pass 2: rows of B_p^{-1}[:, row_e] (e ascending) as CSR (selection inputs) and sliced ELL
    // by row (x_B warm start of the LP kernel), written in place
    const size_t kz = std::max<size_t>(kcnt[P], 1), ez = std::max<size_t>(ecnt[P], 1);
    std::vector<int> kp((size_t)P * (m + 1)), ks((size_t)P * (R + 1)), cap(P + 1);
    int *ke = c->stage[STG_ELEM_KE].reserve<int>(kz), *ki = c->stage[STG_ELEM_KIX].reserve<int>(ez);
    double *kr = c->stage[STG_ELEM_KRAW].reserve<double>(kz), *kv = c->stage[STG_ELEM_KV].reserve<double>(ez);
    if (!ke || !ki || !kr || !kv) return fail(TWOSD_E_DEVICE, "pool elements: pinned staging allocation failed");
    for (int p = 0; p <= P; ++p) cap[p] = (int)ccnt[p];
    parallel_for(P, [&](int p) {
        const PoolBasis &B = c->bp.bases[p];
        const int *rc = rowcnt.data() + (size_t)p * m;
        std::vector<std::pair<int, double>> row;
        size_t at = kcnt[p];
        const size_t e_row0 = ecnt[p] / 64;   // first ELL entry row of this basis
        size_t so = 0;                        // slot offset (entry rows) within the basis
        for (int t = 0; t <= R; ++t) {
            ks[(size_t)p * (R + 1) + t] = (int)(e_row0 + so);
            if (t < R) so += width[(size_t)p * R + t];
        }
        for (int i = 0; i < m; ++i) {
            row.clear();
            for (int q = B.rptr[i]; q < B.rptr[i + 1]; ++q)
                for (int e : bycol[B.rcol[q]]) row.push_back({e, B.rval[q]});
            std::sort(row.begin(), row.end());
            kp[(size_t)p * (m + 1) + i] = (int)at;
            for (auto &ev : row) { ke[at] = ev.first; kr[at] = ev.second; ++at; }
        }
        kp[(size_t)p * (m + 1) + m] = (int)at;
        (void)rc;
        for (int t = 0; t < R; ++t) {
            const int w = width[(size_t)p * R + t];
            const size_t r0 = (size_t)ks[(size_t)p * (R + 1) + t];
            for (int l = 0; l < 64; ++l) {
                const int i = 64 * t + l;
                const int q0 = i < m ? kp[(size_t)p * (m + 1) + i] : 0, q1 = i < m ? kp[(size_t)p * (m + 1) + i + 1] : 0;
                for (int e = 0; e < w; ++e) {
                    const bool has = q0 + e < q1;
                    ki[(r0 + e) * 64 + l] = has ? ke[q0 + e] : 0;
                    kv[(r0 + e) * 64 + l] = has ? kr[q0 + e] : 0.0;
                }
            }
        }
    });
    const auto t_pe1 = std::chrono::steady_clock::now();
    int rc;
    PoolDev &d = c->bp.d;
    if (c->CH > 0 && ((rc = d.kslot.upload_reserve(ks)) || (rc = d.kix.upload_reserve(ki, ecnt[P])) ||
                      (rc = d.kv.upload_reserve(kv, ecnt[P]))))
        return rc;
    const auto t_pe2 = std::chrono::steady_clock::now();
    if (c->CH > 0 && P > 1) {
        // device selection-stream inputs: CSR rows of every basis, and a static record capacity
        // per basis (every row active: m row starts + all its entries)
        if ((rc = d.kp.upload_reserve(kp)) || (rc = d.ke.upload_reserve(ke, kz)) || (rc = d.kraw.upload_reserve(kr, kz)) ||
            (rc = c->d_sel_ptr.upload_reserve(cap)) || (rc = reserve_selection(c, P, cap[P])))
            return rc;
    }
    pool_elements_ready(c);
    if (getenv("TWOSD_DEBUG")) {
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "prepare_elements P=%d: build %.1f ms, upload ell %.1f ms (%zu entries), selection inputs %.1f ms\n",
                P, ms(t_pe0, t_pe1), ms(t_pe1, t_pe2), ecnt[P], ms(t_pe2, std::chrono::steady_clock::now()));
    }
    return TWOSD_OK;
}

// x_B of every pool basis at b: xbase[p][i] = sum_q B_p^{-1}[i][col_q] b[col_q] over the CSR
// rows (pool-strided brptr, MP + 1 per basis; rows >= m are empty), q ascending
__global__ void pool_xbase_kernel(int P, int MP, const int *__restrict__ brptr, const int *__restrict__ brcol,
                                  const double *__restrict__ brval, const double *__restrict__ b, double *__restrict__ xbase) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)P * MP) return;
    const size_t p = t / MP, i = t - p * MP;
    const int *rp = brptr + p * (MP + 1);
    double s = 0.0;
    int q = rp[i];
    const int q1 = rp[i + 1];
    // four entries' loads in flight together; the fmas stay in column order (same bits)
    for (; q + 4 <= q1; q += 4) {
        const int c0 = brcol[q], c1 = brcol[q + 1], c2 = brcol[q + 2], c3 = brcol[q + 3];
        const double v0 = brval[q], v1 = brval[q + 1], v2 = brval[q + 2], v3 = brval[q + 3];
        const double b0 = b[c0], b1 = b[c1], b2 = b[c2], b3 = b[c3];
        s = fma(v0, b0, s);
        s = fma(v1, b1, s);
        s = fma(v2, b2, s);
        s = fma(v3, b3, s);
    }
    for (; q < q1; ++q) s = fma(brval[q], b[brcol[q]], s);
    xbase[t] = s;
}

// primal infeasibility of a basic variable at value x (h_infeas of lp_hyper.hip, tolerance 1e-9)
__device__ __forceinline__ double dev_infeas(double x, int bt) {
    const double tol = 1e-9;
    if (bt == BT_Y || bt == BT_L) return x < -tol ? x : 0.0;
    if (bt == BT_G) return x > tol ? x : 0.0;
    return fabs(x) > tol ? x : 0.0;
}

// Selection stream of one pool basis per block (prepare_x, per x; hb0 = head * 4 + bound type): the rows of basis p that can
// turn infeasible on the training box of the deltas, ordered by their worst box infeasibility
// (largest first, row index on ties), each written as a row-start record (sign-folded
// x_B,i, the sentinel offset k * 65 * 8) followed by its element entries (e, B_p^{-1}[i][row_e]) at the basis's static capacity
// offset; rows without entries add their constant infeasibility to cinf[p] (fixed-order sum).
constexpr int kSelStreamThreads = 256;
// count weight of the selection key in units of the mean |coef_e| E|V_e - E V_e| (storm: 13.5;
// 1M bench: 0 -> 111.5 ms per step, 0.37 - 0.74 -> 105.5 - 105.8, 1.5 -> 112, 3 -> 115; ssn: no effect)
constexpr double kSelCountWeight = 0.5;
constexpr int kSelStreamRows = 1024;   // MP <= 1024 (R <= 16)
__global__ void __launch_bounds__(kSelStreamThreads) pool_selstream_kernel(
    int m, int MP, int k, const double *__restrict__ xbase, const int *__restrict__ hb0,
    const int *__restrict__ kp, const int *__restrict__ ke, const double *__restrict__ kraw, const double *__restrict__ xaux,
    int box, int order_rows, float cw, const int *__restrict__ scap, int2 *__restrict__ rec, int *__restrict__ send,
    float *__restrict__ cinf) {
    __shared__ double skey[kSelStreamRows];
    __shared__ int sidx[kSelStreamRows];
    __shared__ int soff[kSelStreamRows];
    __shared__ float cpart[kSelStreamThreads];
    __shared__ int tsum[kSelStreamThreads];
    const int p = blockIdx.x, tid = threadIdx.x;
    const double *coef = xaux + m, *lo_e = xaux + m + k, *hi_e = xaux + m + 2 * k;
    const int *kpp = kp + (size_t)p * (m + 1);
    float cf = 0.0f;
    for (int i = tid; i < kSelStreamRows; i += kSelStreamThreads) {
        double key = INFINITY;   // inactive rows sort last
        if (i < m) {
            const int t = (hb0[(size_t)p * MP + i] & 3);
            const double xv = xbase[(size_t)p * MP + i];
            const int q0 = kpp[i], q1 = kpp[i + 1];
            if (q0 == q1) {
                const double f = fabs(dev_infeas(xv, t));
                cf += (float)f + (f > 0.0 ? cw : 0.0f);
            } else {
                double worst = 0.0;
                bool active = true;
                if (box) {
                    double lo = xv, hi = xv, mag = fabs(xv);
                    for (int q = q0; q < q1; ++q) {
                        const int e = ke[q];
                        const double g = coef[e] * kraw[q];
                        const double a = g * lo_e[e], bb = g * hi_e[e];
                        lo += fmin(a, bb);
                        hi += fmax(a, bb);
                        mag += fmax(fabs(a), fabs(bb));
                    }
                    const double tol = 1e-9 + 1e-12 * mag;
                    const bool feasible_box = (t == BT_Y || t == BT_L) ? lo > tol : (t == BT_G) ? hi < -tol : false;
                    if (isfinite(lo) && isfinite(hi) && feasible_box) active = false;
                    worst = (t == BT_Y || t == BT_L) ? -lo : (t == BT_G) ? hi : fmax(fabs(lo), fabs(hi));
                    if (!isfinite(worst)) worst = HUGE_VAL;
                }
                if (active) key = order_rows ? -worst : 0.0;
            }
        }
        skey[i] = key;
        sidx[i] = i;
    }
    cpart[tid] = cf;
    __syncthreads();
    // bitonic sort of (key, row) ascending: (-worst, i) lexicographic = the host's stable sort
    for (int kk = 2; kk <= kSelStreamRows; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t2 = tid; t2 < kSelStreamRows / 2; t2 += kSelStreamThreads) {
                const int a = 2 * j * (t2 / j) + (t2 % j), b2 = a + j;
                const bool up = (a & kk) == 0;
                const double ka = skey[a], kb = skey[b2];
                const int ia = sidx[a], ib = sidx[b2];
                const bool gt = ka > kb || (ka == kb && ia > ib);
                if (gt == up) {
                    skey[a] = kb; skey[b2] = ka;
                    sidx[a] = ib; sidx[b2] = ia;
                }
            }
            __syncthreads();
        }
    }
    // records per sorted position, exclusive scan (4 consecutive positions per thread)
    constexpr int PER = kSelStreamRows / kSelStreamThreads;
    int loc[PER], run = 0;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int sp = tid * PER + u;
        const int i = sidx[sp];
        const int c = skey[sp] != INFINITY ? (1 + kpp[i + 1] - kpp[i]) * ((hb0[(size_t)p * MP + i] & 3) == BT_E ? 2 : 1) : 0;
        loc[u] = run;
        run += c;
    }
    tsum[tid] = run;
    __syncthreads();
    if (tid == 0) {   // fixed-order sums: 256 partials (records, constant-row infeasibility)
        int acc = 0;
        float cacc = 0.0f;
        for (int t = 0; t < kSelStreamThreads; ++t) {
            const int v = tsum[t];
            tsum[t] = acc;
            acc += v;
            cacc += cpart[t];
        }
        send[p] = scap[p] + acc;
        cinf[p] = cacc;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; ++u) soff[tid * PER + u] = tsum[tid] + loc[u];
    __syncthreads();
    // emit: one wave per sorted row at a time, the row's entries written by consecutive lanes
    const int lane = tid & 63, wv = tid >> 6;
    const size_t base = (size_t)scap[p];
    for (int sp = wv; sp < kSelStreamRows; sp += kSelStreamThreads / 64) {
        if (skey[sp] == INFINITY) break;   // sorted: the inactive rows are all at the end
        const int i = sidx[sp];
        const int q0 = kpp[i], q1 = kpp[i + 1];
        int2 *out = rec + base + soff[sp];
        // records are sign-folded so that the kernels' test is always "x' > tol": x' = -x for
        // Y / L basics (infeasible below 0), x for G (above 0); a fixed (E) basic is written
        // twice, with +x and -x (|x| > tol <=> one of them > tol)
        const int t = hb0[(size_t)p * MP + i] & 3;
        const int ncopy = t == BT_E ? 2 : 1;
        for (int cpy = 0; cpy < ncopy; ++cpy) {
            const float sg = (t == BT_Y || t == BT_L || cpy == 1) ? -1.0f : 1.0f;
            int2 *o = out + cpy * (1 + q1 - q0);
            // record (value bits, byte offset of the element's staged pair row e * 65 * 8; row start: the
            // offset of row k, which the selection kernels keep zeroed)
            if (lane == 0) o[0] = make_int2(__float_as_int(sg * (float)xbase[(size_t)p * MP + i]), k * 65 * 8);
            for (int q = q0 + lane; q < q1; q += 64) o[1 + q - q0] = make_int2(__float_as_int(sg * (float)kraw[q]), ke[q] * 65 * 8);
        }
    }
}

// per-x shared data: b = r - T x; per pool basis xbase_p = B_p^{-1} b (sparse rows);
// coef_e(x); with a pool, the
// selection stream (active rows that can turn infeasible on the training box of the deltas).
// Every pool basis is independent, so the per-basis work runs on host threads.
int twosd::prepare_x(twosd_ctx *c, const double *x) {
    const int m = c->L.m, MP = c->MP, k = c->k, n1 = c->n1;
    if (c->prep_valid && c->prep_x.size() == (size_t)n1 && (n1 == 0 || std::equal(c->prep_x.begin(), c->prep_x.end(), x)))
        return TWOSD_OK;
    int rc;
    const auto t_start = std::chrono::steady_clock::now();
    if (!c->bp.k_valid && (rc = prepare_elements(c))) return rc;
    std::vector<double> b;
    rhs_at(c, x, nullptr, b);
    const int P = (int)c->bp.bases.size();
    std::vector<double> coef(std::max(k, 1), 1.0);
    for (int e = 0; e < k; ++e) coef[e] = c->pos_col[e] < 0 ? 1.0 : -x[c->pos_col[e]];
    if ((rc = c->d_xbase.fit((size_t)P * MP))) return rc;
    if (c->CH > 0) {
        // everything per x on the device: one upload of [b, coef, box lo, box hi], x_B of every
        // pool basis, then the selection stream (pool_selstream_kernel)
        const bool sel = P > 1;
        const bool box = !c->sel_lo.empty();
        std::vector<double> aux((size_t)m + 3 * (size_t)k, 0.0);
        std::copy(b.begin(), b.end(), aux.begin());
        std::copy(coef.begin(), coef.begin() + k, aux.begin() + m);
        if (box) {
            std::copy(c->sel_lo.begin(), c->sel_lo.end(), aux.begin() + m + k);
            std::copy(c->sel_hi.begin(), c->sel_hi.end(), aux.begin() + m + 2 * k);
        }
        // re-uploaded in place: no reallocation per x
        if ((rc = c->d_xaux.fit(aux.size())) || (rc = c->d_xaux.copy_from(aux.data(), aux.size())) ||
            (rc = c->d_kcoef.fit(coef.size())) || (rc = c->d_kcoef.copy_from(coef.data(), coef.size())))
            return rc;
        const size_t tot = (size_t)P * MP;
        const PoolArrays pa = pool_arrays(c);
        hipLaunchKernelGGL(pool_xbase_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, P, MP, pa.brptr,
                           pa.brcol, pa.brval, c->d_xaux, c->d_xbase);
        HIPCHK(hipGetLastError());
        if (sel) {
            if (MP > kSelStreamRows) return fail(TWOSD_E_UNSUPPORTED, "pool selection: m = %d rows > %d", m, kSelStreamRows);
            // count weight of the selection key: kSelCountWeight x the mean over the random elements
            // of |coef_e(x)| E|V_e - E V_e| (one infeasible row is worth about half a typical
            // scenario perturbation), 0 without distributions.  The same on every rank.
            double sc = 0.0;
            if (c->has_dist && k > 0) {
                for (int e = 0; e < k; ++e) sc += fabs(coef[e]) * c->dist_mad[e];
                sc /= k;
            }
            c->sel_cw = (float)(kSelCountWeight * sc);
            if (const char *e = getenv("TWOSD_SEL_CW")) c->sel_cw = (float)atof(e);   // selection-key experiments
            static const bool sel_order = !getenv("TWOSD_SEL_ROWORDER") || atoi(getenv("TWOSD_SEL_ROWORDER")) != 0;   // A/B knob
            hipLaunchKernelGGL(pool_selstream_kernel, dim3(P), dim3(kSelStreamThreads), 0, c->stream, m, MP, k, c->d_xbase,
                               pa.hb0, pa.kp, pa.ke, pa.kraw, c->d_xaux, box ? 1 : 0, sel_order ? 1 : 0,
                               c->sel_cw, c->d_sel_ptr, reinterpret_cast<int2 *>(c->d_sel_code.p), c->d_sel_end, c->d_sel_cinf);
            HIPCHK(hipGetLastError());
        }
        if (getenv("TWOSD_DEBUG") && sel) {
            HIPCHK(hipStreamSynchronize(c->stream));
            std::vector<int> beg(P + 1), end(P);
            HIPCHK(hipMemcpy(beg.data(), c->d_sel_ptr, sizeof(int) * (P + 1), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(end.data(), c->d_sel_end, sizeof(int) * P, hipMemcpyDeviceToHost));
            c->sel_nnz = 0;
            for (int p = 0; p < P; ++p) c->sel_nnz += end[p] - beg[p];
        }
    }
    c->prep_x.assign(x, x + n1);
    c->prep_valid = true;
    if (getenv("TWOSD_DEBUG")) {
        HIPCHK(hipStreamSynchronize(c->stream));
        fprintf(stderr, "prepare_x: P=%d %.3f ms (%lld selection records)\n", P,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(),
                (long long)c->sel_nnz);
    }
    return TWOSD_OK;
}

// candidate lists from the picks of the training scenarios (any order): the ncand bases the flat
// selection picks most often among the scenarios of each level-1 pick (ties: lower index)
static int set_candidates(twosd_ctx *c, int level1, int ncand, int n, const int *p1, const int *pf) {
    // the differing (level-1 pick, flat pick) pairs bucketed by level-1 pick (counting sort), then
    // per bucket the flat picks sorted and counted by runs; the ncand most frequent kept (ties:
    // lower basis)
    std::vector<int> start(level1 + 1, 0);
    for (int s = 0; s < n; ++s)
        if (pf[s] != p1[s] && p1[s] >= 0 && p1[s] < level1) ++start[p1[s] + 1];
    for (int p = 0; p < level1; ++p) start[p + 1] += start[p];
    std::vector<int> fill(start.begin(), start.end() - 1), bucket(start[level1]);
    for (int s = 0; s < n; ++s)
        if (pf[s] != p1[s] && p1[s] >= 0 && p1[s] < level1) bucket[fill[p1[s]]++] = pf[s];
    std::vector<int> cand((size_t)level1 * ncand, -1);
    std::vector<std::pair<int, int>> v;   // (-count, basis) of one level-1 pick
    for (int p = 0; p < level1; ++p) {
        int *b0 = bucket.data() + start[p], *b1 = bucket.data() + start[p + 1];
        if (b0 == b1) continue;
        std::sort(b0, b1);
        v.clear();
        for (int *a = b0; a < b1;) {
            int *b = a;
            while (b < b1 && *b == *a) ++b;
            v.push_back({-(int)(b - a), *a});
            a = b;
        }
        const size_t nk = std::min<size_t>(v.size(), ncand);
        std::partial_sort(v.begin(), v.begin() + nk, v.end());
        for (size_t i = 0; i < nk; ++i) cand[(size_t)p * ncand + i] = v[i].second;
    }
    if (getenv("TWOSD_DEBUG")) {
        int diff = 0, filled = 0;
        for (int s = 0; s < n; ++s) diff += pf[s] != p1[s];
        for (int v : cand) filled += v >= 0;
        fprintf(stderr, "pool candidates: P=%zu level1=%d: %d of %d training picks change, %d candidate slots filled\n",
                c->bp.bases.size(), level1, diff, n, filled);
    }
    int rc;
    int *h = c->stage[STG_CAND].reserve<int>(cand.size());
    if (!h) return fail(TWOSD_E_DEVICE, "pool candidates: pinned staging allocation failed");
    std::copy(cand.begin(), cand.end(), h);
    if ((rc = c->d_cand.reserve(cand.size()))) return rc;
    HIPCHK(hipMemcpyAsync(c->d_cand, h, sizeof(int) * cand.size(), hipMemcpyHostToDevice, c->stream));
    c->pool_l1 = level1;
    c->pool_ncand = ncand;
    c->cand_pending = false;
    return TWOSD_OK;
}

// Warm-start selection for scenarios [0, N) at the prepared x: pick[s] = pool basis, and
// c->d_order = the scenarios grouped by pick (stable).  Flat: least key over the whole pool.
// Two-level (pool_l1 > 0): least key over pool[0, pool_l1), then over the candidates of that
// pick.  npool_override > 0: flat over pool[0, npool_override) (candidate training).
int twosd::select_pool(twosd_ctx *c, const double *d_dv, int N, int *d_pick, int npool_override) {
    const int P = (int)c->bp.bases.size();
    const bool two = npool_override <= 0 && c->pool_l1 > 0 && c->pool_l1 < P && c->pool_ncand > 0 && (c->d_cand || c->cand_pending);
    const int np1 = npool_override > 0 ? npool_override : two ? c->pool_l1 : P;
    int rc;
    size_t tb = 0, tb2 = 0;
    HIPCHK(sort_by_pool(d_pick, nullptr, N, P, nullptr, &tb, c->stream));
    HIPCHK(sort_by_pool(d_pick, nullptr, N, np1, nullptr, &tb2, c->stream));
    tb = std::max(tb, tb2);
    if ((size_t)N > c->d_order.cap || tb > c->d_sort_tmp.cap) {   // both at once, as one workspace
        if ((rc = c->d_order.alloc((size_t)N)) || (rc = c->d_sort_tmp.alloc(tb))) return rc;
    }
    if (two && (rc = c->d_sel_key.fit((size_t)N))) return rc;
    // partials of the chunked selections (small batches: several pool chunks per scenario tile)
    const int g1 = pool_select_split(N, np1), g2 = two ? pool_refine_split(N, c->pool_ncand) : 1;
    const size_t pneed = (size_t)std::max(g1, g2) * N;
    if (std::max(g1, g2) > 1 && ((rc = c->d_sel_pkey.fit(pneed)) || (rc = c->d_sel_ppick.fit(pneed)))) return rc;
    PoolSelParams S{};
    S.N = N; S.k = c->k; S.npool = np1; S.dv = d_dv;
    S.kcoef = c->d_kcoef;
    S.cinf = c->d_sel_cinf; S.sptr = c->d_sel_ptr; S.send = c->d_sel_end; S.rec = reinterpret_cast<const int2 *>(c->d_sel_code.p);
    S.pick = d_pick;
    S.cw = c->sel_cw;
    S.key = two ? c->d_sel_key : nullptr;
    S.pkey = g1 > 1 ? c->d_sel_pkey : nullptr;
    S.ppick = g1 > 1 ? c->d_sel_ppick : nullptr;
    HIPCHK(launch_pool_select(S, c->stream));
    if (two && c->cand_pending &&
        (rc = set_candidates(c, c->cand_pl1, c->cand_pnc, (int)c->cand_p1.size(), c->cand_p1.data(), c->cand_pf.data())))
        return rc;
    if (two) {
        HIPCHK(sort_by_pool(d_pick, c->d_order, N, np1, c->d_sort_tmp, &tb, c->stream));
        PoolRefineParams Q{};
        Q.N = N; Q.k = c->k; Q.ncand = c->pool_ncand; Q.dv = d_dv; Q.kcoef = c->d_kcoef;
        Q.cinf = c->d_sel_cinf; Q.sptr = c->d_sel_ptr; Q.send = c->d_sel_end; Q.rec = S.rec;
        Q.order = c->d_order; Q.cand = c->d_cand; Q.pick = d_pick; Q.key = c->d_sel_key; Q.cw = c->sel_cw;
        Q.pkey = g2 > 1 ? c->d_sel_pkey : nullptr;
        Q.pci = g2 > 1 ? c->d_sel_ppick : nullptr;
        HIPCHK(launch_pool_refine(Q, c->stream));
    }
    HIPCHK(sort_by_pool(d_pick, c->d_order, N, P, c->d_sort_tmp, &tb, c->stream));
    return TWOSD_OK;
}

// flat and level-1 picks of training scenarios [first, first + count) of epi at x
static int candidate_picks(twosd_ctx *c, const EpiDevice &E, const double *x, int first, int count, int level1,
                           int *p1, int *pf) {
    int rc;
    if ((rc = prepare_x(c, x))) return rc;
    if ((rc = c->d_cpick.reserve((size_t)count))) return rc;   // grow-only: no reallocation per refresh
    int *d_p = c->d_cpick;
    const double *dv = E.d_dv + (size_t)first * c->k;
    auto picks = [&](int np, int *out) {   // selection runs on c->stream
        int r = select_pool(c, dv, count, d_p, np);
        if (!r && (hipStreamSynchronize(c->stream) != hipSuccess ||
                   hipMemcpy(out, d_p, sizeof(int) * count, hipMemcpyDeviceToHost) != hipSuccess))
            r = fail(TWOSD_E_DEVICE, "pool candidates: selection failed");
        return r;
    };
    rc = picks(level1, p1);
    if (!rc) rc = picks((int)c->bp.bases.size(), pf);
    return rc;
}

// the lists are built by the next two-level selection (select_pool), on the host while its
// level-1 pass runs on the device: same lists, the host time off the critical path
static int defer_candidates(twosd_ctx *c, int level1, int ncand, std::vector<int> &&p1, std::vector<int> &&pf) {
    c->cand_p1 = std::move(p1);
    c->cand_pf = std::move(pf);
    c->cand_pl1 = level1;
    c->cand_pnc = ncand;
    c->cand_pending = true;
    c->pool_l1 = level1;
    c->pool_ncand = ncand;
    return TWOSD_OK;
}

extern "C" int twosd_pool_candidate_picks(twosd_ctx *c, int epi, const double *x, int first, int count, int level1, int *p1,
                                          int *pf) {
    if (!c || !c->bp.has_basis) return fail(TWOSD_E_STATE, "pool_candidate_picks: no primary basis");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "pool_candidate_picks: epigraph %d does not exist", epi);
    const EpiDevice &E = c->epis[epi];
    const int P = (int)c->bp.bases.size();
    if (first < 0 || count < 1 || first + count > E.count || level1 < 1 || level1 >= P || !p1 || !pf || (c->n1 > 0 && !x) ||
        c->CH <= 0)
        return fail(TWOSD_E_ARG, "pool_candidate_picks: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    reset_candidates(c);   // the flat pick runs over the whole pool
    return candidate_picks(c, E, x, first, count, level1, p1, pf);
}

extern "C" int twosd_pool_set_candidates(twosd_ctx *c, int level1, int ncand, int n, const int *p1, const int *pf) {
    if (!c || !c->bp.has_basis) return fail(TWOSD_E_STATE, "pool_set_candidates: no primary basis");
    const int P = (int)c->bp.bases.size();
    if (level1 < 1 || level1 >= P || ncand < 1 || ncand > 1024 || n < 0 || (n > 0 && (!p1 || !pf)))
        return fail(TWOSD_E_ARG, "pool_set_candidates: bad arguments");
    for (int s = 0; s < n; ++s)
        if (p1[s] < 0 || p1[s] >= P || pf[s] < 0 || pf[s] >= P) return fail(TWOSD_E_ARG, "pool_set_candidates: pick outside the pool");
    HIPCHK(hipSetDevice(c->device));
    return defer_candidates(c, level1, ncand, std::vector<int>(p1, p1 + n), std::vector<int>(pf, pf + n));
}

// Two-level selection from training scenarios [first, first + count) of epigraph epi at x:
// level 1 = pool[0, level1) (the most frequent bases); the candidates of a level-1 basis p are
// the ncand bases that the flat selection over the whole pool picks most often for training
// scenarios whose level-1 pick is p (ties: lower index).  level1 = 0 back to flat selection.
extern "C" int twosd_pool_build_candidates(twosd_ctx *c, int epi, const double *x, int first, int count, int level1,
                                           int ncand) {
    if (!c || !c->bp.has_basis) return fail(TWOSD_E_STATE, "pool_build_candidates: no primary basis");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "pool_build_candidates: epigraph %d does not exist", epi);
    const EpiDevice &E = c->epis[epi];
    const int P = (int)c->bp.bases.size();
    if (first < 0 || count < 1 || first + count > E.count || level1 < 0 || ncand < 0 || ncand > 1024 || (c->n1 > 0 && !x))
        return fail(TWOSD_E_ARG, "pool_build_candidates: bad arguments");
    reset_candidates(c);
    if (level1 == 0 || ncand == 0 || level1 >= P || P < 2 || c->CH <= 0) return TWOSD_OK;   // flat selection
    HIPCHK(hipSetDevice(c->device));
    std::vector<int> p1(count), pf(count);
    int rc;
    if ((rc = candidate_picks(c, E, x, first, count, level1, p1.data(), pf.data()))) return rc;
    return defer_candidates(c, level1, ncand, std::move(p1), std::move(pf));
}

extern "C" int twosd_last_pool_picks(twosd_ctx *c, int N, int *picks) {
    if (!c || !picks || N < 0 || N > c->last.N) return fail(TWOSD_E_ARG, "last_pool_picks: bad arguments");
    if (c->bp.bases.size() <= 1 || !c->d_pool_pick) {
        std::fill(picks, picks + N, 0);
        return TWOSD_OK;
    }
    HIPCHK(hipMemcpy(picks, c->d_pool_pick, sizeof(int) * N, hipMemcpyDeviceToHost));
    return TWOSD_OK;
}

extern "C" int twosd_invalidate_x(twosd_ctx *c) {
    if (!c) return fail(TWOSD_E_ARG, "invalidate_x: NULL context");
    c->prep_valid = false;   // (the cut's PK rows do not depend on x: kept)
    return TWOSD_OK;
}
