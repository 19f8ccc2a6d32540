// reform.hip -- the stage every cut re-formed from stored picks shares.  The
// bootstrap (boot_kernel.hip: weights c_b(s) q_s, M + 1 rows per handle) and the tail cut (risk.hip:
// 1[score_s > eta] q_s, one row) each stream the deltas with a kernel of their own and meet here
// with per-vertex integer weights, shard partials of S and a total weight W per row; S, g and the
// normalised cut are formed here, in reform_layout.h's layouts.  No floating-point atomics.
//
// Not here, on purpose: the streaming kernels boot_reform_kernel<KE, GM, LIST> and
// risk_treform_kernel<KE>, and the histogram kernels boot_hist_kernel<GR, LIST> and
// risk_thist_kernel.  The bootstrap's walk over a tail handle's list is an instantiation (LIST) of
// its kernels over all scenarios: one body each.  Every bit of S depends on how the compiler
// contracts wq * PK * dv + acc and the bootstrap kernel sits at 191 VGPRs, so the rule for any
// change to these bodies is: each instantiation's instruction stream and kernel descriptor equal
// the parent commit's, compared on the CPU (tools/isa_same.py; profiles/reform_merge) -- equal
// streams give equal bits and equal speed, and a difference is not to be argued away.  risk.hip's
// two kernels remain separate kernels: they form one row, skip the scenarios outside the tail (a
// skipped scenario's row is never loaded) and flag a scenario by its score, not by a list, so no
// instantiation of the bootstrap's bodies has their instruction stream.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include "reform.h"

namespace twosd {

constexpr int kReformRB = 8;   // rows per block of reform_g_kernel

// 256 / NSEG outputs per block; segment g adds chunks [g per, (g + 1) per) in chunk order from 0.0,
// then the segments are added in order from 0.0 (NSEG = 1: 0.0 + s is s, a sum from +0.0 is never -0.0)
template <int NSEG>
__global__ void __launch_bounds__(256) reform_sum_kernel(int nchunks, int width, const double *__restrict__ slots,
                                                         double *__restrict__ out) {
    constexpr int PB = 256 / NSEG;
    __shared__ double sh[NSEG][PB];
    const int li = threadIdx.x % PB, seg = threadIdx.x / PB;
    const int idx = blockIdx.x * PB + li;
    const int per = (nchunks + NSEG - 1) / NSEG;
    const int c0 = seg * per, c1 = min(nchunks, c0 + per);
    double s = 0.0;
    if (idx < width)
        for (int c = c0; c < c1; ++c) s += slots[(size_t)c * width + idx];
    sh[seg][li] = s;
    __syncthreads();
    if (seg != 0 || idx >= width) return;
    double t = 0.0;
#pragma unroll
    for (int g = 0; g < NSEG; ++g) t += sh[g][li];
    out[idx] = t;
}

// gpart[c][b][i] = sum_{v in vertex chunk c} hist[b][v] V[v][i] for rows b0 .. b0 + 7 (blockIdx.y)
__global__ void __launch_bounds__(256) reform_g_kernel(int nv, int nvs, int m, int chunk, int B,
                                                       const unsigned long long *__restrict__ hist, const double *__restrict__ V,
                                                       double *__restrict__ gpart) {
    const int b0 = blockIdx.y * kReformRB;
    const int v0 = blockIdx.x * chunk, v1 = min(nv, v0 + chunk);
    for (int i = threadIdx.x; i < m; i += 256) {
        double acc[kReformRB];
#pragma unroll
        for (int r = 0; r < kReformRB; ++r) acc[r] = 0.0;
        for (int v = v0; v < v1; ++v) {
            if (hist[v] == 0ull) continue;   // row 0 weighs every picked vertex: no other row weighs v
            const double x = V[(size_t)v * m + i];
#pragma unroll
            for (int r = 0; r < kReformRB; ++r)
                if (b0 + r < B) acc[r] = fma((double)hist[(size_t)(b0 + r) * nvs + v], x, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < kReformRB; ++r)
            if (b0 + r < B) gpart[((size_t)blockIdx.x * B + b0 + r) * m + i] = acc[r];
    }
}

// one block per row b of one handle: g = sum of the vertex chunks (chunk order), then reform.h's alpha,
// beta and weight_mark at index b * H + j.  gs: the LP's rows, twosd_set_template refuses more than 64 * 16
__global__ void __launch_bounds__(256) reform_cut_kernel(int B, int H, int j, int m, int n1, int k, int nbc,
                                                         const double *__restrict__ gpart, const double *__restrict__ r,
                                                         const double *__restrict__ T, const int *__restrict__ col,
                                                         const double *__restrict__ S, const unsigned long long *__restrict__ Wq,
                                                         double wunit, double c0, double *__restrict__ alpha,
                                                         double *__restrict__ beta, double *__restrict__ wm) {
    __shared__ double gs[1024];
    __shared__ double as;
    const int b = blockIdx.x;
    const size_t o = (size_t)b * H + j;
    double *bo = beta + o * n1;
    const unsigned long long wq = Wq[b];
    if (wq == 0ull) {
        for (int jj = threadIdx.x; jj < n1; jj += 256) bo[jj] = 0.0;
        if (threadIdx.x == 0) { alpha[o] = 0.0; wm[o] = 0.0; }
        return;
    }
    for (int i = threadIdx.x; i < m; i += 256) {
        double s = 0.0;
        for (int c = 0; c < nbc; ++c) s += gpart[((size_t)c * B + b) * m + i];
        gs[i] = s;
    }
    __syncthreads();
    for (int jj = threadIdx.x; jj < n1; jj += 256) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) s = fma(T[(size_t)i * n1 + jj], gs[i], s);
        bo[jj] = -s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int i = 0; i < m; ++i) a = fma(gs[i], r[i], a);
        for (int e = 0; e < k; ++e) {
            const double se = S[(size_t)b * k + e];
            if (col[e] < 0) a += se;
            else bo[col[e]] -= se;
        }
        as = a;
    }
    __syncthreads();
    const double inv = 1.0 / (double)wq;
    for (int jj = threadIdx.x; jj < n1; jj += 256) bo[jj] *= inv;
    if (threadIdx.x == 0) {
        alpha[o] = as * inv + c0;
        wm[o] = (double)wq * wunit;
    }
}

int reform_prepare(twosd_ctx *c, int B, int H, int nvs) {
    ReformState &S = c->reform;
    int rc;
    if (!S.tmpl_ready) {
        std::vector<int> col(std::max(c->k, 1), -1);
        for (int e = 0; e < c->k; ++e) col[e] = c->pos_col[e];
        std::vector<double> T = c->T;
        if (T.empty()) T.push_back(0.0);
        if ((rc = S.d_T.upload(T)) || (rc = S.d_r.upload(c->r)) || (rc = S.d_col.upload(col))) return rc;
        S.tmpl_ready = true;
    }
    const size_t rows = (size_t)B * H;
    if ((rc = S.out.fit(rows * (2 + (size_t)c->n1)))) return rc;
    S.d_alpha = S.out; S.d_wm = S.out + rows; S.d_beta = S.out + 2 * rows;
    // vertex chunks hold 32 vertices or more: a bound on every handle's chunk count
    return S.gpart.fit((size_t)std::max(1, (nvs + 31) / 32) * B * c->L.m);
}

void reform_sum_shards(twosd_ctx *c, bool eight_segments, int nchunks, int width, const double *slots, double *out) {
    if (eight_segments)
        hipLaunchKernelGGL(reform_sum_kernel<8>, dim3((width + 31) / 32), dim3(256), 0, c->stream, nchunks, width, slots, out);
    else
        hipLaunchKernelGGL(reform_sum_kernel<1>, dim3((width + 255) / 256), dim3(256), 0, c->stream, nchunks, width, slots, out);
}

int reform_finalize_block(twosd_ctx *c, int B, int H, int j, int nv, int nvs, const unsigned long long *hist, const double *S,
                          const unsigned long long *Wq, double wunit) {
    ReformState &R = c->reform;
    const ReformVertexChunks vc = reform_vertex_chunks(nv);
    const int m = c->L.m;
    hipLaunchKernelGGL(reform_g_kernel, dim3(vc.nbc, (B + kReformRB - 1) / kReformRB), dim3(256), 0, c->stream, nv, nvs, m, vc.chunk, B,
                       hist, c->dvs.V, R.gpart.p);
    hipLaunchKernelGGL(reform_cut_kernel, dim3(B), dim3(256), 0, c->stream, B, H, j, m, c->n1, c->k, vc.nbc, R.gpart.p, R.d_r.p,
                       R.d_T.p, R.d_col.p, S, Wq, wunit, c->has_bounds ? c->c0 : 0.0, R.d_alpha, R.d_beta, R.d_wm);
    HIPCHK(hipGetLastError());
    return TWOSD_OK;
}

}  // namespace twosd
