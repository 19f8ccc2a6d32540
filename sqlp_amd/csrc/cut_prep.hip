// cut_prep.hip -- the cut's operands (the maths: cut_kernel.hip).  Per vertex set: PK / PKT / PKO
// gathers and the twin links (update_pk).  Per epigraph: the running max |dv| (cut_fold_dmax).  Per
// cut at x (cut_operand_stage): the vertex bases and decision bands, the pass, the argmax's vertex
// list and the chunk sources of the three passes.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <algorithm>
#include <vector>
#include "cut_common.h"

namespace twosd {

__global__ void cut_pk_kernel(int from, int to, int m, int k, int k4, int vcap, const int *__restrict__ rows,
                              const int *__restrict__ eord, const double *__restrict__ V, double *__restrict__ PK,
                              double *__restrict__ PKT, double *__restrict__ PKO) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = (to - from) * k4;
    if (idx >= total) return;
    const int v = from + idx / k4, e = idx % k4;
    const double x = e < k ? V[(size_t)v * m + rows[e]] : 0.0;
    PK[(size_t)v * k4 + e] = x;
    PKT[(size_t)e * vcap + v] = x;
    PKO[(size_t)v * k4 + e] = e < k ? V[(size_t)v * m + rows[eord[e]]] : 0.0;   // column q = e in the restated order
}

// Twin vertices.  Two vertices whose PK rows are bit-identical have bit-identical restated dot
// terms t for every scenario, so at an x where their bases are equal too their restated scores
// are equal for every scenario: the lower index wins under both rules (the first strict maximum;
// the lowest index within the tie window), and the higher one can never be picked.  storm's
// duals come in such groups (vertices differing only on rows where r - T x is 0), and each one
// made every scenario it won an exact tie the fixup had to re-decide.  tprev[v] is the previous
// vertex of v's PK-equality group (-1: none), maintained with PK; cut_pktc_kernel drops a vertex
// whose base equals that of an earlier group member at this x (cut_compact_kernel).
__global__ void cut_twin_hash_kernel(int from, int to, int k4, const double *__restrict__ PK, unsigned long long *__restrict__ phash) {
    const int v = from + blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= to) return;
    unsigned long long h = 0x9e3779b97f4a7c15ull;
    for (int e = 0; e < k4; ++e) {
        h ^= (unsigned long long)__double_as_longlong(PK[(size_t)v * k4 + e]) + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
        h *= 0xff51afd7ed558ccdull;
    }
    phash[v] = h;
}

__global__ void cut_iota_kernel(int *v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}

// tprev[v] = the highest u < v with PK row u bit-identical to PK row v (one wavefront per vertex)
__global__ void __launch_bounds__(256) cut_twin_prev_kernel(int from, int to, int k4, const double *__restrict__ PK,
                                                            const unsigned long long *__restrict__ phash, int *__restrict__ tprev) {
    const int lane = threadIdx.x & 63;
    const int v = from + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (v >= to) return;   // wave-uniform
    const unsigned long long hv = phash[v];
    int best = -1;
    for (int u = v - 1 - lane; u >= 0 && best < 0; u -= 64) {
        if (phash[u] != hv) continue;
        bool same = true;
        for (int e = 0; e < k4 && same; ++e)
            same = __double_as_longlong(PK[(size_t)u * k4 + e]) == __double_as_longlong(PK[(size_t)v * k4 + e]);
        if (same) best = u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
    if (lane == 0) tprev[v] = best;
}

// The argmax's vertex list at x: every vertex except the dominated twins (v whose base equals
// that of an earlier member of its PK-equality group), ascending, so that the MFMA pass does no
// work for them and "lowest index" keeps its meaning.  One block; tprev == nullptr keeps all.
__global__ void __launch_bounds__(1024) cut_compact_kernel(int nv, const double *__restrict__ base, const int *__restrict__ tprev,
                                                           int *__restrict__ vmap, int *__restrict__ nvc,
                                                           unsigned long long *__restrict__ ntwin) {
    __shared__ int wsum[16];
    __shared__ int off;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (threadIdx.x == 0) off = 0;
    __syncthreads();
    for (int v0 = 0; v0 < nv; v0 += 1024) {
        const int v = v0 + threadIdx.x;
        bool keep = v < nv;
        if (keep && tprev) {
            const double b = base[v];
            for (int u = tprev[v]; u >= 0; u = tprev[u])   // tprev[u] < u: the walk ends
                if (base[u] == b) { keep = false; break; }
        }
        const unsigned long long bal = __ballot(keep);
        const int pos = __popcll(bal & ((1ull << lane) - 1));
        if (lane == 0) wsum[wid] = __popcll(bal);
        __syncthreads();
        int before = off;
        for (int w = 0; w < wid; ++w) before += wsum[w];
        if (keep) vmap[before + pos] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
            for (int w = 0; w < 16; ++w) t += wsum[w];
            off += t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *nvc = off;
        if (ntwin) *ntwin = (unsigned long long)(nv - off);
    }
}

// The same links for all vertices at once from the (hash, vertex) pairs sorted by hash (stable:
// vertices ascending within a hash): the previous entry of a run with a bit-identical row is the
// highest lower twin.  O(nv log nv) instead of cut_twin_prev_kernel's O(nv^2) for a rebuild.
__global__ void cut_twin_sorted_kernel(int nv, int k4, const double *__restrict__ PK, const unsigned long long *__restrict__ hs,
                                       const int *__restrict__ vs, int *__restrict__ tprev) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const int v = vs[i];
    int prev = -1;
    for (int j = i - 1; j >= 0 && hs[j] == hs[i]; --j) {   // runs are short (twin groups)
        const int u = vs[j];
        bool same = true;
        for (int e = 0; e < k4 && same; ++e)
            same = __double_as_longlong(PK[(size_t)u * k4 + e]) == __double_as_longlong(PK[(size_t)v * k4 + e]);
        if (same) { prev = u; break; }
    }
    tprev[v] = prev;
}

// PKOc[c] = PKO[vmap[c]], basec[c] = base[vmap[c]] for c < nvc: the fixup works on the argmax's
// positions (its logs hold them), so its candidate loads need no translation
__global__ void cut_compact_rows_kernel(int nv, int k4, const int *__restrict__ vmap, const int *__restrict__ nvc_p,
                                        const double *__restrict__ PKO, const double *__restrict__ base,
                                        double *__restrict__ PKOc, double *__restrict__ basec, int vcap32, float *__restrict__ basec32) {
    const int nvc = *nvc_p;
    // basec32[c] = the least float >= base[vmap[c]] (-inf past nvc): an upper bound of the base, so
    // the fp32 prefilter of cut_argmax3_kernel never rejects a score the fp64 test would accept
    if (basec32)
        for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < vcap32; c += gridDim.x * blockDim.x)
            basec32[c] = c < nvc ? __double2float_ru(base[vmap[c]]) : -INFINITY;
    const size_t total = (size_t)nv * k4;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx / k4), q = (int)(idx % k4);
        if (c >= nvc) continue;
        const int v = vmap[c];
        PKOc[idx] = PKO[(size_t)v * k4 + q];
        if (q == 0) basec[c] = base[v];
    }
}

// PKTc[kk][c] = coef_kk * PKT[kk][vmap[c]] over rows [0, rows) x columns [0, vcap32), zero
// outside [0, k) x [0, nvc) (the LDS-DMA source of cut_argmax2_kernel; per x).
// With base != nullptr, row k holds base[vmap[c]] (-inf for c >= nvc): the MFMA then adds the
// vertex base through a constant 1 in the scenarios' delta column k.
// PKTc32 (rows32 rows, may be null): the element rows of PKTc rounded to fp32, zero past k (the
// fp32 pass adds the base in fp64 outside the MFMA)
__global__ void cut_pktc_kernel(int k, int rows, int vcap, int vcap32, const double *__restrict__ PKT,
                                const double *__restrict__ coef, const double *__restrict__ base, const int *__restrict__ vmap,
                                const int *__restrict__ nvc_p, double *__restrict__ PKTc, int rows32, float *__restrict__ PKTc32) {
    const int nvc = *nvc_p;
    const size_t total = (size_t)std::max(rows, PKTc32 ? rows32 : 0) * vcap32;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int kk = (int)(idx / vcap32), c = (int)(idx % vcap32);
        const int v = c < nvc ? vmap[c] : 0;
        const double pc = (kk < k && c < nvc) ? coef[kk] * PKT[(size_t)kk * vcap + v] : 0.0;
        double x = pc;
        if (base && kk == k) x = c < nvc ? base[v] : -INFINITY;
        if (kk < rows) PKTc[idx] = x;
        if (PKTc32 && kk < rows32) PKTc32[idx] = (float)pc;
    }
}

// base[v] = sum_i V[v][i] * bvec[i] in index order with every product and sum rounded on its
// own (oracle_build_cut's vb[v]), one wavefront per vertex: the lanes form the products of a
// 512-entry slice in LDS, lane 0 adds them in order.  The wave also folds the vertex's term of
// the decision band: |base[v]| + sum_e |PK[v,e] coef_e| dmax_e (any order: a bound).
constexpr int kVbSlice = 512;
__global__ void __launch_bounds__(256) cut_vbase_kernel(int nv, int m, int k, int k4, const double *__restrict__ V,
                                                        const double *__restrict__ bvec, const double *__restrict__ PK,
                                                        const double *__restrict__ coef, const unsigned long long *__restrict__ dmax,
                                                        double *__restrict__ base, unsigned long long *__restrict__ band_bits,
                                                        double band_scale, double band_scale32) {
#pragma clang fp contract(off)
    __shared__ double prod[4][kVbSlice];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int v0 = blockIdx.x * 4; v0 < nv; v0 += gridDim.x * 4) {   // block-uniform trip count
        const int v = v0 + wid;
        const bool act = v < nv;
        const double *p = V + (size_t)(act ? v : 0) * m;
        double s = 0.0;
        for (int i0 = 0; i0 < m; i0 += kVbSlice) {
            const int n = min(kVbSlice, m - i0);
            if (act)
                for (int i = lane; i < n; i += 64) prod[wid][i] = p[i0 + i] * bvec[i0 + i];
            __syncthreads();
            if (act && lane == 0) {
#pragma unroll 8
                for (int i = 0; i < n; ++i) s = s + prod[wid][i];
            }
            __syncthreads();
        }
        if (!act) continue;
        double a = 0.0, pm = 0.0, dm = 0.0, um = 0.0;
        for (int e = lane; e < k; e += 64) {
            const double pc = fabs(PK[(size_t)v * k4 + e] * coef[e]), de = __longlong_as_double((long long)dmax[e]);
            a += pc * de;
            pm = fmax(pm, pc);
            dm = fmax(dm, de);
            um = fmax(um, ldexp(pc, ci8::scale_exp(de)));   // |u_e| = |pc_e| 2^E_e (cut_i8.h)
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o);
            pm = fmax(pm, __shfl_xor(pm, o));
            dm = fmax(dm, __shfl_xor(dm, o));
            um = fmax(um, __shfl_xor(um, o));
        }
        // the integer pass's vertex scale (the value cut_pkq_kernel forms) and normalised operand sum
        const int Sv = ci8::scale_exp(um);
        double ns = 0.0;
        for (int e = lane; e < k; e += 64) {
            const double pc = fabs(PK[(size_t)v * k4 + e] * coef[e]), de = __longlong_as_double((long long)dmax[e]);
            const int Ee = ci8::scale_exp(de);
            ns += ldexp(de, -Ee) + ldexp(pc, Ee - Sv);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ns += __shfl_xor(ns, o);
        if (lane == 0) {
            base[v] = s;
            const double t = fabs(s) + a;
            // the band itself (a positive scale keeps the order of the maxima, rounding included)
            const double b64 = isfinite(t) ? band_scale * t : INFINITY;
            atomicMax(band_bits + BAND_F64, (unsigned long long)__double_as_longlong(b64));
            // the fp32 pass: the element terms rounded to fp32 and summed by an fmaf chain (the f32
            // MFMA's arithmetic) differ from the exact dot by at most gamma_{k+2}(u32) a, plus
            // 2^-126 (1 + max|PK coef| + max dmax) per term for operands and partial sums below
            // the normal range; scale32 = 4 gamma_{k+4}(u32) doubles that bound as band_scale does.
            // The base stays fp64 (the restatement's own value), so the fp64 band is added.
            const double b32 = b64 + band_scale32 * a + 4.0 * (k + 4) * ldexp(1.0, -126) * (1.0 + pm + dm);
            atomicMax(band_bits + BAND_F32, (unsigned long long)__double_as_longlong(isfinite(b32) ? b32 : INFINITY));
            // operands and sums well inside the fp32 range, or the cut runs the fp64 pass
            const double lim = ldexp(1.0, 100);
            if (!(a < lim && pm < lim && dm < lim)) atomicOr(band_bits + BAND_F32_RANGE, 1ull);
            // the integer pass: ci8::band_term bounds |t - sum_e pc_e dv_e| for its score term t
            // (operand quantisation, dropped limb pairs, the level combination's fp32 roundings);
            // doubled as the others, and the base and the final add stay fp64: the fp64 band is added
            const double bi8 = b64 + 2.0 * ci8::band_term(k, Sv, ns);
            atomicMax(band_bits + BAND_I8, (unsigned long long)__double_as_longlong(isfinite(bi8) ? bi8 : INFINITY));
        }
    }
}

// the cut's pass: a reduced-precision pass when asked and every vertex's operands fit
// (band_bits[BAND_F32_RANGE] == 0), else fp64; band_bits[BAND_ACTIVE] = that pass's band (what every
// later kernel of the cut reads), [BAND_PASS] = the pass.
// The integer pass (2) replaces the fp32 one when asked (wanti8), no delta seen so far was NaN
// or infinite (*nonfinite == 0, folded with dmax) and its band is finite.
__global__ void cut_band_select_kernel(unsigned long long *band_bits, int want32, int wanti8,
                                       const unsigned long long *__restrict__ nonfinite) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long m = (want32 && band_bits[BAND_F32_RANGE] == 0) ? 1ull : 0ull;
    if (m && wanti8 && *nonfinite == 0 && isfinite(__longlong_as_double((long long)band_bits[BAND_I8]))) m = 2ull;
    band_bits[BAND_ACTIVE] = m == 2 ? band_bits[BAND_I8] : m ? band_bits[BAND_F32] : band_bits[BAND_F64];
    band_bits[BAND_PASS] = m;
}

// dmax[e] = max |dv[s][e]| over scenarios [from, to) folded into the epigraph's running maximum
// (non-negative doubles order as their bit patterns); dmax[k] != 0: some delta was NaN or infinite
__global__ void __launch_bounds__(256) cut_dmax_kernel(int from, int to, int k, const double *__restrict__ dv,
                                                       unsigned long long *__restrict__ dmax) {
    if ((int)threadIdx.x >= k) return;
    const int e = threadIdx.x;
    double mx = 0.0;
    bool bad = false;
    for (int s = from + blockIdx.x; s < to; s += gridDim.x) {
        const double d = dv[(size_t)s * k + e];
        mx = fmax(mx, fabs(d));   // NaN ignored: its scores never win
        bad |= !isfinite(d);
    }
    atomicMax(&dmax[e], (unsigned long long)__double_as_longlong(mx));
    if (bad) atomicOr(&dmax[k], 1ull);   // a non-finite delta seen: the integer pass is not used (cut_band_select_kernel)
}

// the limb planes of the compacted vertices at x, their output scales, and (block 0) the deltas'
// quantisation factors.  One block per chunk: thread (q, vv) = (t >> 5, t & 31) owns the 16
// elements e = 16 q + b of vertex position c = 32 chunk + vv.
__global__ void __launch_bounds__(256) cut_pkq_kernel(int k, int KS, int vcap, const double *__restrict__ PKT,
                                                      const double *__restrict__ coef, const unsigned long long *__restrict__ dmax,
                                                      const int *__restrict__ vmap, const int *__restrict__ nvc_p,
                                                      int8_t *__restrict__ PKq, float *__restrict__ scq, double *__restrict__ dsc) {
    __shared__ double smax[8][32];
    const int t = threadIdx.x, vv = t & 31, q = t >> 5;
    const int c = blockIdx.x * 32 + vv;
    const bool act = q < 4 * KS, in = c < *nvc_p;
    const int v = in ? vmap[c] : 0;
    if (blockIdx.x == 0 && t < 128)
        dsc[t] = t < k ? ldexp(1.0, ci8::kQ - ci8::scale_exp(__longlong_as_double((long long)dmax[t]))) : 0.0;
    double pc[16];
    int Ee[16];
    double mx = 0.0;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        const int e = 16 * q + b;
        pc[b] = 0.0;
        Ee[b] = 0;
        if (act && in && e < k) {
            pc[b] = coef[e] * PKT[(size_t)e * vcap + v];
            Ee[b] = ci8::scale_exp(__longlong_as_double((long long)dmax[e]));
            mx = fmax(mx, fabs(ldexp(pc[b], Ee[b])));
        }
    }
    smax[q][vv] = mx;
    __syncthreads();
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) mx = fmax(mx, smax[qq][vv]);
    const int S = ci8::scale_exp(mx);
    if (q == 0) scq[c] = in ? ldexpf(1.0f, S + ci8::kOutShift) : 0.0f;
    if (!act) return;
    unsigned wd[ci8::kL][4] = {};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        int8_t lb[ci8::kL];
        ci8::limbs(ci8::quantise(pc[b], S - Ee[b]), lb);   // u_e = pc_e 2^E_e at scale S: one exact scaling
#pragma unroll
        for (int l = 0; l < ci8::kL; ++l) wd[l][b >> 2] |= (unsigned)(uint8_t)lb[l] << (8 * (b & 3));
    }
    int8_t *img = PKq + (size_t)blockIdx.x * i8_chunk_bytes(KS);
#pragma unroll
    for (int l = 0; l < ci8::kL; ++l) {
        i4 o = {(int)wd[l][0], (int)wd[l][1], (int)wd[l][2], (int)wd[l][3]};
        *reinterpret_cast<i4 *>(img + i8_frag_off(KS, l, q >> 2, q & 3, vv)) = o;
    }
}

// bring PK/PKT up to date with the vertex set
int update_pk(twosd_ctx *c) {
    CutWs *w = cws(c);
    const int nv = c->dvs.size, k = c->k, k4 = (std::max(k, 1) + 3) & ~3, m = c->L.m;
    int rc;
    if (!w->rows || w->pk_k4 != k4 || w->m != m) {
        if ((rc = w->rows.alloc(std::max(k, 1))) || (rc = w->eord.alloc(std::max(k, 1)))) return rc;
        if (k) HIPCHK(hipMemcpy(w->rows, c->pos_row.data(), sizeof(int) * k, hipMemcpyHostToDevice));
        // the restated score's element order: ascending row (the dense dot over the m rows); within a
        // row the RHS element (column -1) first, then the T columns ascending -- the canonical order of
        // twosd_ref._element_terms, whatever order the caller listed the positions in (no position
        // is listed twice, twosd_set_random_positions, so this is a total order)
        std::vector<int> ord(k);
        for (int e = 0; e < k; ++e) ord[e] = e;
        std::sort(ord.begin(), ord.end(), [&](int a, int b) {
            return c->pos_row[a] != c->pos_row[b] ? c->pos_row[a] < c->pos_row[b] : c->pos_col[a] < c->pos_col[b];
        });
        if (k) HIPCHK(hipMemcpy(w->eord, ord.data(), sizeof(int) * k, hipMemcpyHostToDevice));
        w->pk_count = 0;
        w->pk_k4 = k4;
        w->m = m;
    }
    if (nv > w->pk_vcap) {
        const int vcap = std::max(nv, 2 * w->pk_vcap + 256);
        if ((rc = w->PK.alloc((size_t)vcap * k4)) || (rc = w->PKT.alloc((size_t)vcap * k4)) ||
            (rc = w->PKO.alloc((size_t)vcap * k4)) || (rc = w->phash.alloc(vcap)) ||
            (rc = w->tprev.alloc(vcap)))
            return rc;
        w->pk_vcap = vcap;
        w->pk_count = 0;
    }
    if (w->pk_count > nv) w->pk_count = 0;
    if (w->pk_count < nv) {
        const int total = (nv - w->pk_count) * k4;
        hipLaunchKernelGGL(cut_pk_kernel, dim3((total + 255) / 256), dim3(256), 0, c->stream, w->pk_count, nv, m, k, k4,
                           w->pk_vcap, w->rows, w->eord, c->dvs.V, w->PK, w->PKT, w->PKO);
        HIPCHK(hipGetLastError());
        const int nn = nv - w->pk_count;
        hipLaunchKernelGGL(cut_twin_hash_kernel, dim3((nn + 255) / 256), dim3(256), 0, c->stream, w->pk_count, nv, k4, w->PK,
                           w->phash);
        if ((long long)nn * nv <= (1ll << 22)) {   // a few new vertices: scan the earlier ones
            hipLaunchKernelGGL(cut_twin_prev_kernel, dim3((nn + 3) / 4), dim3(256), 0, c->stream, w->pk_count, nv, k4, w->PK,
                               w->phash, w->tprev);
        } else {                                             // a rebuild: sort every vertex by hash
            if ((rc = w->tw_hs.fit(nv)) || (rc = w->tw_vin.fit(nv)) || (rc = w->tw_vout.fit(nv))) return rc;
            size_t need = 0;
            HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, w->phash.p, w->tw_hs.p, w->tw_vin.p, w->tw_vout.p, nv, 0, 64, c->stream));
            if ((rc = w->tw_tmp.fit(need))) return rc;
            hipLaunchKernelGGL(cut_iota_kernel, dim3((nv + 255) / 256), dim3(256), 0, c->stream, w->tw_vin, nv);
            // (the earlier vertices' hashes are kept in phash; only the new ones were hashed above)
            HIPCHK(hipcub::DeviceRadixSort::SortPairs(w->tw_tmp.p, need, w->phash.p, w->tw_hs.p, w->tw_vin.p, w->tw_vout.p, nv, 0, 64,
                                                      c->stream));
            hipLaunchKernelGGL(cut_twin_sorted_kernel, dim3((nv + 255) / 256), dim3(256), 0, c->stream, nv, k4, w->PK, w->tw_hs,
                               w->tw_vout, w->tprev);
        }
        HIPCHK(hipGetLastError());
        w->pk_count = nv;
    }
    return TWOSD_OK;
}

int cut_ray_operands(twosd_ctx *c, const double *x, int J, const double *d_F, double *PK, double *PKT, double *PKO, double *base,
                     unsigned long long *scratch, const double **coef, const int **eord, int *k4_out) {
    CutWs *w = cws(c);
    const int k = c->k, m = c->L.m;
    int rc;
    if ((rc = update_pk(c))) return rc;   // the element rows and their order (and V's own gathers)
    const int k4 = w->pk_k4;
    if ((rc = cut_size_vectors(w, m))) return rc;
    host_bvec_coef(c, x, k4, w->h_bvec, w->h_coef);
    HIPCHK(hipMemcpyAsync(w->coef, w->h_coef.data(), sizeof(double) * k4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(w->bvec, w->h_bvec.data(), sizeof(double) * m, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(scratch, 0, sizeof(unsigned long long) * (k + 1 + BAND_COUNT), c->stream));
    hipLaunchKernelGGL(cut_pk_kernel, dim3((J * k4 + 255) / 256), dim3(256), 0, c->stream, 0, J, m, k, k4, J, w->rows, w->eord, d_F, PK,
                       PKT, PKO);
    hipLaunchKernelGGL(cut_vbase_kernel, dim3(std::max(1, std::min((J + 3) / 4, 4096))), dim3(256), 0, c->stream, J, m, k, k4, d_F,
                       w->bvec, PK, w->coef, scratch, base, scratch + k + 1, 0.0, 0.0);
    HIPCHK(hipGetLastError());
    *coef = w->coef;
    *eord = w->eord;
    *k4_out = k4;
    return TWOSD_OK;
}

int cut_fold_dmax(twosd_ctx *c, int epi, int N, int k) {
    CutWs *w = cws(c);
    int rc;
    if ((int)w->dmax.size() <= epi) {
        w->dmax.resize(epi + 1);
        w->dmax_rows.resize(epi + 1, 0);
        w->dmax_k.resize(epi + 1, -1);
    }
    // Invariant: an epigraph's scenario rows are append-only (twosd_add_scenarios /
    // twosd_add_sampled_scenarios append; no entry point rewrites or removes rows), so the
    // cached max folds in only rows [dmax_rows, N).  A row count below the cached one can only
    // mean the rows were replaced: fold everything in again (a too-small dmax would narrow the
    // decision band and mark near-tied rows decided without a fixup).
    if (w->dmax_k[epi] != k || w->dmax_rows[epi] > N) {
        // k maxima and the non-finite flag (entry k)
        if ((rc = w->dmax[epi].alloc(std::max(k, 1) + 1))) return rc;
        HIPCHK(hipMemsetAsync(w->dmax[epi], 0, sizeof(unsigned long long) * (std::max(k, 1) + 1), c->stream));
        w->dmax_k[epi] = k;
        w->dmax_rows[epi] = 0;
    }
    if (w->dmax_rows[epi] < N && k > 0) {
        const int rows = N - w->dmax_rows[epi];
        hipLaunchKernelGGL(cut_dmax_kernel, dim3(std::max(1, std::min(rows, 2048))), dim3(256), 0, c->stream, w->dmax_rows[epi], N, k,
                           c->epis[epi].d_dv, w->dmax[epi]);
        w->dmax_rows[epi] = N;
    }
    return TWOSD_OK;
}

void cut_operand_stage(twosd_ctx *c, int epi, const CutShape &sh, const CutPlan &pl, bool twins) {
    CutWs *w = cws(c);
    const int nv = sh.nv, k = sh.k, k4 = pl.k4, vcap32 = pl.vcap32;
    hipLaunchKernelGGL(cut_vbase_kernel, dim3(std::max(1, std::min((nv + 3) / 4, 4096))), dim3(256), 0, c->stream, nv, c->L.m, k, k4,
                       c->dvs.V, w->bvec, w->PK, w->coef, w->dmax[epi], w->base, w->band_bits, pl.band_scale, pl.band_scale32);
    hipLaunchKernelGGL(cut_band_select_kernel, dim3(1), dim3(64), 0, c->stream, w->band_bits, pl.want32 ? 1 : 0, pl.wanti8 ? 1 : 0,
                       w->dmax[epi] + k);
    hipLaunchKernelGGL(cut_compact_kernel, dim3(1), dim3(1024), 0, c->stream, nv, w->base, twins ? w->tprev : nullptr, w->vmap,
                       w->nvc, w->fstats + CS_TWINS);
    const size_t tot2 = (size_t)std::max(pl.rows, pl.rows32) * vcap32;
    hipLaunchKernelGGL(cut_pktc_kernel, dim3((unsigned)std::min<size_t>(4096, (tot2 + 255) / 256)), dim3(256), 0, c->stream, k,
                       pl.rows, w->pk_vcap, vcap32, w->PKT, w->coef, w->base, w->vmap, w->nvc, w->PKTc, pl.rows32,
                       pl.want32 ? w->PKTc32 : nullptr);
    hipLaunchKernelGGL(cut_compact_rows_kernel, dim3((unsigned)std::min<size_t>(2048, ((size_t)nv * k4 + 255) / 256)), dim3(256), 0,
                       c->stream, nv, k4, w->vmap, w->nvc, w->PKO, w->base, w->PKOc, w->basec, vcap32,
                       pl.want32 ? w->basec32 : nullptr);
    w->i8_ks = 0;
    if (pl.wanti8) {
        hipLaunchKernelGGL(cut_pkq_kernel, dim3(vcap32 / 32), dim3(256), 0, c->stream, k, pl.KS8, w->pk_vcap, w->PKT, w->coef,
                           w->dmax[epi], w->vmap, w->nvc, w->PKq, w->scq, w->dsc);
        w->i8_ks = pl.KS8;
    }
}

}  // namespace twosd
