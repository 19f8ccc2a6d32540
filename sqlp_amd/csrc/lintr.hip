// lintr.hip -- correlated continuous elements on the device (SMPS BLOCKS LINTR):
// every member of a LINTR block is v = c + H xi over a few independent latent variables.
//
// draw_scenarios is the one way the library draws a batch.  For a context with LINTR blocks it
//   1. runs the main pass (launch_sample_plan over the k elements).  A LINTR member has kind 4,
//      which the sampler kernels read as UNIFORM(0, 0): a don't-care value in the member's slot that
//      step 3 overwrites later on the same stream.  Skipped when every element is a LINTR member;
//   2. per chunk of N_c scenarios (whole groups of the plan), draws the Q latents with the same
//      kBlocks = true kernels on a SampleParams that describes them as an independent layout:
//      k := Q, tmpl := 0, element word elead[l] = k + l, no kind-3 entry (so no block table is
//      touched), out := the scratch N_c x Q.  v - 0 is v bit for bit, so the scratch holds columns
//      k .. k+Q-1 of a k + Q element layout;
//   3. lintr_apply_kernel forms the members of the chunk from the scratch.
// The scratch is bounded (64 MiB by default), so the chunking is invisible in the stream: every
// value is a function of (seed, global index, latent, plan, tables) only.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include "twosd_ctx.h"

namespace twosd {

// One thread per (scenario, member row), the member fastest across the lanes: the lanes of one
// scenario read the same row of the latent scratch (one or two lines, served from L2 / the vector
// cache) and neighbouring CSR rows.  No LDS.  Products and sums are single roundings in the
// contract's order.  They are written as plain * and + under `fp contract(off)`, the idiom of
// restated_score in cut_fixup.hip: __dadd_rn(v, __dmul_rn(h, xi)) compiles to v_fmac_f64 here (the
// intrinsics are inline * and + that carry the default contraction with them, whatever the caller's
// pragma says); the loop's ISA is now one v_mul_f64 and one v_add_f64.
__global__ void __launch_bounds__(256) lintr_apply_kernel(LintrParams P) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)P.N * P.M) return;
    const int s = (int)(idx / P.M), m = (int)(idx - (long long)s * P.M);
    const double *xi = P.xi + (size_t)s * P.Q;
    double v = P.c[m];
    for (int p = P.rptr[m], end = P.rptr[m + 1]; p < end; ++p) v = v + P.h[p] * xi[P.col[p]];
    const int e = P.elem[m];
    P.out[(size_t)s * P.k + e] = v - P.tmpl[e];   // stored as the delta, like the sampler kernels
}

hipError_t launch_lintr_apply(const LintrParams &P, hipStream_t st) {
    const long long total = (long long)P.N * P.M;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(lintr_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, P);
    return hipGetLastError();
}

int upload_lintr(twosd_ctx *c, const LintrTables &T) {
    c->has_lintr = false;
    c->lintr_M = c->lintr_Q = 0;
    if (T.M == 0) {
        c->d_lt_elem.release(); c->d_lt_rptr.release(); c->d_lt_col.release(); c->d_lt_c.release(); c->d_lt_h.release();
        c->d_lt_kind.release(); c->d_lt_off.release(); c->d_lt_word.release(); c->d_lt_val.release(); c->d_lt_prob.release();
        c->d_lt_p0.release(); c->d_lt_p1.release(); c->d_lt_zero.release(); c->d_lt_xi.release();
        return TWOSD_OK;
    }
    int rc;
    if ((rc = c->d_lt_elem.upload(T.elem)) || (rc = c->d_lt_rptr.upload(T.rptr)) || (rc = c->d_lt_col.upload(T.col)) ||
        (rc = c->d_lt_c.upload(T.c)) || (rc = c->d_lt_h.upload(T.h)) || (rc = c->d_lt_kind.upload(T.lkind)) ||
        (rc = c->d_lt_off.upload(T.loff)) || (rc = c->d_lt_word.upload(T.lword)) || (rc = c->d_lt_val.upload(T.lval)) ||
        (rc = c->d_lt_prob.upload(T.lprob)) || (rc = c->d_lt_p0.upload(T.lp0)) || (rc = c->d_lt_p1.upload(T.lp1)) ||
        (rc = c->d_lt_zero.upload(std::vector<double>((size_t)T.Q, 0.0))))
        return rc;
    c->lintr_M = T.M;
    c->lintr_Q = T.Q;
    c->has_lintr = true;
    return TWOSD_OK;
}

// scenarios per chunk of the latent pass: what 64 MiB of scratch hold, in whole groups (at least one)
static int64_t lintr_chunk_size(int Q, int G) {
    int64_t chunk = std::max<int64_t>(((int64_t)64 << 20) / ((int64_t)sizeof(double) * std::max(Q, 1)), 1);
    if (const char *e = getenv("TWOSD_LINTR_CHUNK")) chunk = std::min<int64_t>(std::max<int64_t>(atoll(e), 1), 1 << 24);   // test hook
    return std::max<int64_t>(chunk / G * G, G);
}

int draw_scenarios(twosd_ctx *c, int n, uint64_t seed, uint64_t first_index, double *out, int mode, int G) {
    if (n <= 0) return TWOSD_OK;
    if (!c->has_lintr || c->lintr_M < c->k) HIPCHK(launch_sample_plan(sample_params(c, n, seed, first_index, out), mode, G, c->stream));
    if (!c->has_lintr) return TWOSD_OK;
    const int Q = c->lintr_Q, k = c->k;
    const int64_t chunk = std::min<int64_t>(lintr_chunk_size(Q, G), n);
    if (int rc = c->d_lt_xi.fit((size_t)chunk * Q)) return rc;
    for (int64_t at = 0; at < n; at += chunk) {
        const int nc = (int)std::min<int64_t>(chunk, n - at);
        SampleParams L{};
        L.N = nc; L.k = Q; L.seed = seed; L.first_index = first_index + (uint64_t)at;
        L.kind = c->d_lt_kind; L.off = c->d_lt_off; L.val = c->d_lt_val; L.prob = c->d_lt_prob;
        L.p0 = c->d_lt_p0; L.p1 = c->d_lt_p1; L.tmpl = c->d_lt_zero; L.out = c->d_lt_xi;
        L.blocks = true;                  // the instantiations that read the element word from elead
        L.elead = c->d_lt_word;
        HIPCHK(launch_sample_plan(L, mode, G, c->stream));
        LintrParams P{};
        P.N = nc; P.k = k; P.M = c->lintr_M; P.Q = Q;
        P.elem = c->d_lt_elem; P.c = c->d_lt_c; P.rptr = c->d_lt_rptr; P.col = c->d_lt_col; P.h = c->d_lt_h;
        P.tmpl = c->d_dist_tmpl; P.xi = c->d_lt_xi; P.out = out + (size_t)at * k;
        HIPCHK(launch_lintr_apply(P, c->stream));
    }
    return TWOSD_OK;
}

}  // namespace twosd
