// feas.hip -- feasibility rays: the ray set F of a context (twosd_fray_*) and the
// ray extraction of a batch (twosd_solve_rays).  The arithmetic of a ray -- snap, normalisation,
// dedup key -- is feas_rays.h, shared with the host function twosd_fray_key.
//
// A stage-2 LP that is infeasible at x ends the dual simplex at a row r with no entering column;
// sigma = +-e_r' B^{-1} is then a Farkas certificate (lp_hyper.hip, the RAY instantiation).  W is not
// random, so the ray certifies every scenario and every x with sigma' b_w(x) > 0.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <unordered_set>
#include <vector>
#include "cut_common.h"
#include "feas_rays.h"
#include "wave_ops.h"

using namespace twosd;

namespace {

constexpr double kRayZero = 1e-12;   // = HPI_ZERO of the LP kernel's recoveries
constexpr int kRayChunk = 4096;      // list positions per re-solve

// raw ray i -> snapped, normalised ray and its key; ok[i] = 0 for an all-zero or non-finite ray.
// One thread per ray: a push is a few hundred rays of at most 1024 entries.
__global__ void fray_prepare_kernel(int count, int mv, const double *__restrict__ in, double *__restrict__ nrm,
                                    unsigned long long *__restrict__ key, int *__restrict__ ok, int *__restrict__ nbad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double *o = nrm + (size_t)i * mv;
    for (int j = 0; j < mv; ++j) o[j] = in[(size_t)i * mv + j];
    fr::snap(o, mv, kRayZero);
    const bool good = fr::normalise(o, mv, o);
    ok[i] = good ? 1 : 0;
    key[i] = good ? fr::key(o, mv) : 0ull;
    if (!good) atomicAdd(nbad, 1);
}

// push in order (one block): a ray whose key is present maps to that index (first occurrence
// kept), a new one is appended.  meta[0] = size (updated only when everything fitted), meta[1] != 0:
// the set would have passed maxn and is unchanged (rows past size are not part of the set).
__global__ void __launch_bounds__(256) fray_insert_kernel(int count, int mv, int maxn, const double *__restrict__ nrm,
                                                          const unsigned long long *__restrict__ key, double *F,
                                                          unsigned long long *keys, int *meta, int *__restrict__ idx) {
    __shared__ int found;
    int size = meta[0];
    bool over = false;
    for (int i = 0; i < count; ++i) {
        if (threadIdx.x == 0) found = 0x7fffffff;
        __syncthreads();
        const unsigned long long k = key[i];
        for (int j = threadIdx.x; j < size; j += blockDim.x)
            if (keys[j] == k) atomicMin(&found, j);
        __syncthreads();
        const int f = found;
        __syncthreads();
        if (f != 0x7fffffff) {
            if (threadIdx.x == 0 && idx) idx[i] = f;
            continue;
        }
        if (size >= maxn) { over = true; break; }   // block-uniform
        for (int j = threadIdx.x; j < mv; j += blockDim.x) F[(size_t)size * mv + j] = nrm[(size_t)i * mv + j];
        if (threadIdx.x == 0) {
            keys[size] = k;
            if (idx) idx[i] = size;
        }
        ++size;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        meta[1] = over ? 1 : 0;
        if (!over) meta[0] = size;
    }
}

// flag[s] = scenario s ended infeasible; cnt[0] += scenarios that ended at the iteration limit or numerically
__global__ void ray_flag_kernel(int N, const int *__restrict__ st, char *__restrict__ flag, int *cnt) {
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < N; s += gridDim.x * blockDim.x) {
        flag[s] = st[s] == TWOSD_LP_INFEASIBLE;
        if (st[s] != TWOSD_LP_INFEASIBLE && st[s] != TWOSD_LP_OPTIMAL) atomicAdd(cnt, 1);
    }
}

// the kept rays of a chunk: sel[u] = list position within the chunk; row o0 + u of the outputs (the
// scenario as an index of the epigraph: the batch starts at `first`)
__global__ void ray_gather_kernel(int U, int m, int o0, int first, const int *__restrict__ sel, const int *__restrict__ list,
                                  const double *__restrict__ ray, const int *__restrict__ ray_row, const int *__restrict__ head,
                                  double *__restrict__ ray_out, int *__restrict__ row_out, int *__restrict__ head_out,
                                  int *__restrict__ scen_out) {
    const size_t tot = (size_t)U * m;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) {
        const int u = (int)(i / m), j = (int)(i % m);
        const size_t src = (size_t)sel[u] * m + j, dst = (size_t)(o0 + u) * m + j;
        ray_out[dst] = ray[src];
        if (head) head_out[dst] = head[src];
        if (j == 0) {
            row_out[o0 + u] = ray_row[sel[u]];
            scen_out[o0 + u] = first + list[sel[u]];
        }
    }
}

int fray_init(twosd_ctx *c) {
    FrayState &S = c->fray;
    const int mv = c->L.m;
    if (S.F && S.mv == mv) return TWOSD_OK;
    int rc;
    if ((rc = S.F.alloc((size_t)TWOSD_FRAY_MAX * mv)) || (rc = S.keys.alloc(TWOSD_FRAY_MAX)) || (rc = S.d_meta.alloc(3))) return rc;
    HIPCHK(hipMemset(S.d_meta, 0, sizeof(int) * 3));
    S.mv = mv;
    S.size = 0;
    return TWOSD_OK;
}

// push count raw rays (device, count x mv) in order; d_idx (device, nullable) their indices.
// Nothing is pushed when one of them is refused or the set would pass TWOSD_FRAY_MAX.
int fray_push_device(twosd_ctx *c, int count, const double *d_rays, int *d_idx) {
    int rc;
    if ((rc = fray_init(c))) return rc;
    if (count == 0) return TWOSD_OK;
    FrayState &S = c->fray;
    const int mv = S.mv;
    if ((rc = S.nrm.fit((size_t)count * mv)) || (rc = S.inkey.fit(count)) || (rc = S.ok.fit(count))) return rc;
    HIPCHK(hipMemsetAsync(S.d_meta + 2, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(fray_prepare_kernel, dim3((count + 63) / 64), dim3(64), 0, c->stream, count, mv, d_rays, S.nrm.p, S.inkey.p,
                       S.ok.p, S.d_meta + 2);
    HIPCHK(hipGetLastError());
    int nbad = 0;
    HIPCHK(hipMemcpyAsync(&nbad, S.d_meta + 2, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (nbad) return fail(TWOSD_E_ARG, "fray_push: %d of %d rays are all zero or not finite; nothing pushed", nbad, count);
    hipLaunchKernelGGL(fray_insert_kernel, dim3(1), dim3(256), 0, c->stream, count, mv, TWOSD_FRAY_MAX, S.nrm.p, S.inkey.p, S.F.p,
                       S.keys.p, S.d_meta.p, d_idx);
    HIPCHK(hipGetLastError());
    int meta[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(meta, S.d_meta, sizeof(meta), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (meta[1]) return fail(TWOSD_E_UNSUPPORTED, "fray_push: the ray set holds at most %d rays; nothing pushed", TWOSD_FRAY_MAX);
    S.size = meta[0];
    return TWOSD_OK;
}


// ---- violation scan.  Score of (ray j, scenario s) at x in the arithmetic of the cut's restated
// score (oracle_build_cut): v_js = base_j + t_js, base_j = sum_i sigma_ji (r - T x)_i in index order
// (cut_vbase_kernel), t_js = sum over the random elements by ascending row of
// sigma_j[row_e] * (coef_e(x) dv[s][e]), every product and every sum rounded on its own.
//
// feas_scan_kernel: scenarios across lanes, 64 per tile; a tile of up to 64 rays' element gathers
// (PKO rows: the restated order) sits in LDS for the whole block, the tile's deltas are staged
// through LDS 32 elements at a time (read along the scenarios' rows, multiplied by coef_e(x),
// transposed with a stride of 65 so that a wave's reads of one element are conflict-free).  The
// block's 8 waves split the rays (ray jj on wave jj % 8): a lane reads its scenario's delta once
// per element and the rays' coefficients as LDS broadcasts.  Per ray the wave keeps the running
// maximum and the lowest scenario attaining it (DPP maximum, ballot, first set bit: lanes are
// ascending scenarios; tiles are visited ascending, so a later equal score never replaces an
// earlier one).  One partial per block and ray; feas_merge_kernel folds the blocks in block order
// with the same rule (greater, or equal at a lower scenario), so the result is the same under any
// grid.  No floating-point atomics.
constexpr int kFsTile = 64;    // scenarios per tile (one per lane)
constexpr int kFsKS = 32;      // elements per staged slice
constexpr int kFsRays = 64;    // rays per tile
constexpr int kFsWaves = 8;
constexpr int kFsKMax = 128;   // the cut's envelope: k <= 127

struct FeasScanParams {
    int N, k, k4;
    int J, j0, nj;            // rays in all, first ray and rays of this tile (nj <= kFsRays)
    const double *dv;         // scenario rows (k doubles each); scenario i is row list[i] (list == nullptr: row i)
    const int *list;
    const double *coef;       // k4: coef_e(x)
    const int *eord;          // k: elements by ascending row
    const double *PKO;        // J x k4: sigma_j[row of element eord[q]]
    const double *base;       // J
    double *pmax;             // gridDim.x x J
    int *parg;
    unsigned char *cut;       // N: some ray scores > 0 (written by the first ray tile, or-ed by the later ones)
};

// U = rays per wave (1, 2 or 8: tiles of up to 8, 16 and 64 rays); the rows of a tile past nj are
// zero (score 0 + 0: never reported, never counted), so the element loop has no branch in it
template <int U>
__global__ void __launch_bounds__(64 * kFsWaves) feas_scan_kernel(FeasScanParams P) {
#pragma clang fp contract(off)
    extern __shared__ double sr[];                 // (U kFsWaves) x k4: the ray tile
    __shared__ double sd[kFsKS * (kFsTile + 1)];   // the deltas of one slice, [element][scenario]
    __shared__ double scf[kFsKMax];                // coef_e(x) and the element of position q, in the restated order
    __shared__ int se[kFsKMax];
    __shared__ unsigned char sc[kFsWaves][kFsTile];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = P.k, k4 = P.k4, nj = P.nj;
    for (int idx = threadIdx.x; idx < U * kFsWaves * k4; idx += blockDim.x)
        sr[idx] = idx < nj * k4 ? P.PKO[(size_t)P.j0 * k4 + idx] : 0.0;
    for (int q = threadIdx.x; q < k; q += blockDim.x) {
        const int e = P.eord[q];
        se[q] = e;
        scf[q] = P.coef[e];
    }
    double bm[U], bs[U];
    int ba[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int jj = u * kFsWaves + wid;
        bm[u] = -INFINITY;
        ba[u] = 0x7fffffff;
        bs[u] = jj < nj ? P.base[P.j0 + jj] : 0.0;
    }
    const double *myr = sr + (size_t)wid * k4;     // ray u of this wave: row u kFsWaves + wid
    const int ntiles = (P.N + kFsTile - 1) / kFsTile;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int s0 = tile * kFsTile;
        const bool valid = s0 + lane < P.N;
        double t[U];
#pragma unroll
        for (int u = 0; u < U; ++u) t[u] = 0.0;
        for (int q0 = 0; q0 < k; q0 += kFsKS) {
            const int kq = min(kFsKS, k - q0);
            __syncthreads();   // the previous slice (and, the first time, the ray tile) is in place / consumed
#pragma unroll 4
            for (int idx = threadIdx.x; idx < kFsTile * kq; idx += 64 * kFsWaves) {
                const int sl = kq == kFsKS ? idx / kFsKS : idx / kq, qq = idx - sl * kq;
                double v = 0.0;
                if (s0 + sl < P.N) {
                    const size_t rowi = P.list ? (size_t)P.list[s0 + sl] : (size_t)(s0 + sl);
                    v = scf[q0 + qq] * P.dv[rowi * k + se[q0 + qq]];
                }
                sd[qq * (kFsTile + 1) + sl] = v;
            }
            __syncthreads();
#pragma unroll 4
            for (int qq = 0; qq < kq; ++qq) {
                const double d = sd[qq * (kFsTile + 1) + lane];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const double p = myr[(size_t)u * kFsWaves * k4 + q0 + qq] * d;
                    t[u] = t[u] + p;
                }
            }
        }
        bool any = false;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int jj = u * kFsWaves + wid;
            if (jj < nj) {   // wave-uniform
                const double v = bs[u] + t[u];
                const double vv = valid ? v : -INFINITY;
                const double M = wmax_any(vv);
                if (M > bm[u]) {
                    const uint64_t hit = __builtin_amdgcn_ballot_w64(vv == M);
                    bm[u] = M;
                    ba[u] = s0 + (int)__builtin_ctzll(hit);
                }
                any |= valid & (v > 0.0);
            }
        }
        sc[wid][lane] = any ? 1 : 0;
        __syncthreads();
        if (threadIdx.x < kFsTile && s0 + (int)threadIdx.x < P.N) {
            unsigned char o = 0;
            for (int w = 0; w < kFsWaves; ++w) o |= sc[w][threadIdx.x];
            if (P.j0 > 0) o |= P.cut[s0 + threadIdx.x];
            P.cut[s0 + threadIdx.x] = o;
        }
        __syncthreads();
    }
    if (lane == 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int jj = u * kFsWaves + wid;
            if (jj < nj) {
                P.pmax[(size_t)blockIdx.x * P.J + P.j0 + jj] = bm[u];
                P.parg[(size_t)blockIdx.x * P.J + P.j0 + jj] = ba[u];
            }
        }
    }
}

template <int U>
hipError_t launch_feas_scan(const FeasScanParams &P, int G, hipStream_t st) {
    static bool attr_set = false;   // the largest tile: 64 rays of 128 elements
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void *)feas_scan_kernel<U>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           U * kFsWaves * kFsKMax * 8);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(feas_scan_kernel<U>, dim3(G), dim3(64 * kFsWaves), sizeof(double) * U * kFsWaves * P.k4, st, P);
    return hipGetLastError();
}

// the blocks' partials in block order: the greater maximum, or an equal one at a lower scenario
__global__ void feas_merge_kernel(int J, int G, int first, const double *__restrict__ pmax, const int *__restrict__ parg,
                                  double *__restrict__ rmax, int *__restrict__ rarg) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= J) return;
    double M = -INFINITY;
    int A = 0x7fffffff;
    for (int b = 0; b < G; ++b) {
        const double v = pmax[(size_t)b * J + j];
        const int a = parg[(size_t)b * J + j];
        if (v > M || (v == M && a < A)) { M = v; A = a; }
    }
    rmax[j] = M;
    rarg[j] = A == 0x7fffffff ? -1 : first + A;
}

__global__ void feas_count_kernel(int N, const unsigned char *__restrict__ cut, unsigned long long *out) {
    unsigned long long a = 0;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < N; s += gridDim.x * blockDim.x) a += cut[s] != 0;
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
    if ((threadIdx.x & 63) == 0 && a) atomicAdd(out, a);   // integers: exact in any order
}

// flag[i] = 1 - cut[i]: the scenarios of a list no ray cuts off
__global__ void feas_keep_kernel(int N, const unsigned char *__restrict__ cut, char *__restrict__ flag) {
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < N; s += gridDim.x * blockDim.x) flag[s] = cut[s] ? 0 : 1;
}

// scan of N scenarios (rows list[i] of d_dv, or rows [0, N)) against J rays (device, J x m) at x:
// S.rmax / S.rarg (J; arg = first + position), S.cut (N), S.ncut[0]
int feas_scan_device(twosd_ctx *c, const double *x, const double *d_rays, int J, const double *d_dv, const int *d_list, int N,
                     int first) {
    FrayState &S = c->fray;
    const int k = c->k, k4 = (std::max(k, 1) + 3) & ~3;
    int rc;
    if ((rc = S.pk.fit((size_t)J * k4)) || (rc = S.pkt.fit((size_t)J * k4)) || (rc = S.pko.fit((size_t)J * k4)) ||
        (rc = S.base.fit(J)) || (rc = S.scratch.fit(k + 1 + BAND_COUNT)) || (rc = S.rmax.fit(J)) || (rc = S.rarg.fit(J)) ||
        (rc = S.cut.fit((size_t)N)) || (rc = S.ncut.fit(1)))
        return rc;
    const double *coef = nullptr;
    const int *eord = nullptr;
    int k4c = 0;
    if ((rc = cut_ray_operands(c, x, J, d_rays, S.pk, S.pkt, S.pko, S.base, S.scratch, &coef, &eord, &k4c))) return rc;
    if (k4c != k4) return fail(TWOSD_E_STATE, "feas_scan: element row length %d != %d", k4c, k4);
    const int ntiles = (N + kFsTile - 1) / kFsTile;
    int G = std::min(ntiles, 4 * c->num_cus);
    if (const char *e = getenv("TWOSD_FEAS_BLOCKS")) G = std::max(1, std::min(ntiles, atoi(e)));   // test knob: the result must not change
    if ((rc = S.pmax.fit((size_t)G * J)) || (rc = S.parg.fit((size_t)G * J))) return rc;
    FeasScanParams P{};
    P.N = N; P.k = k; P.k4 = k4; P.J = J;
    P.dv = d_dv; P.list = d_list; P.coef = coef; P.eord = eord; P.PKO = S.pko; P.base = S.base;
    P.pmax = S.pmax; P.parg = S.parg; P.cut = S.cut;
    HIPCHK(hipEventRecord(c->ev[EV_MARK_0], c->stream));
    for (int j0 = 0; j0 < J; j0 += kFsRays) {   // ray tiles in an outer loop
        P.j0 = j0;
        P.nj = std::min(kFsRays, J - j0);
        if (P.nj <= kFsWaves) HIPCHK(launch_feas_scan<1>(P, G, c->stream));
        else if (P.nj <= 2 * kFsWaves) HIPCHK(launch_feas_scan<2>(P, G, c->stream));
        else HIPCHK(launch_feas_scan<kFsRays / kFsWaves>(P, G, c->stream));
    }
    hipLaunchKernelGGL(feas_merge_kernel, dim3((J + 255) / 256), dim3(256), 0, c->stream, J, G, first, S.pmax.p, S.parg.p, S.rmax.p,
                       S.rarg.p);
    HIPCHK(hipEventRecord(c->ev[EV_MARK_1], c->stream));
    HIPCHK(hipMemsetAsync(S.ncut, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(feas_count_kernel, dim3(std::max(1, std::min(1024, (N + 255) / 256))), dim3(256), 0, c->stream, N, S.cut.p,
                       S.ncut.p);
    HIPCHK(hipGetLastError());
    return TWOSD_OK;
}

// drop from the list S.list[p0, p0 + n) every scenario some ray of d_rays (J x m) cuts off at x; the
// survivors, still ascending, are left at S.list[p0, p0 + *n_out)
int filter_list(twosd_ctx *c, const double *x, const double *d_rays, int J, const double *d_dv, int p0, int n, int *n_out) {
    FrayState &S = c->fray;
    int rc;
    if ((rc = feas_scan_device(c, x, d_rays, J, d_dv, S.list + p0, n, 0))) return rc;
    if ((rc = S.list2.fit((size_t)n)) || (rc = S.flag.fit((size_t)n))) return rc;
    hipLaunchKernelGGL(feas_keep_kernel, dim3(std::max(1, std::min(1024, (n + 255) / 256))), dim3(256), 0, c->stream, n, S.cut.p,
                       S.flag.p);
    size_t need = 0;
    HIPCHK(hipcub::DeviceSelect::Flagged(nullptr, need, S.list.p + p0, S.flag.p, S.list2.p, S.cnt.p + 1, n, c->stream));
    if ((rc = S.tmp.fit(need))) return rc;
    HIPCHK(hipcub::DeviceSelect::Flagged(S.tmp.p, need, S.list.p + p0, S.flag.p, S.list2.p, S.cnt.p + 1, n, c->stream));
    int kept = 0;
    HIPCHK(hipMemcpyAsync(&kept, S.cnt + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (kept) HIPCHK(hipMemcpyAsync(S.list + p0, S.list2, sizeof(int) * kept, hipMemcpyDeviceToDevice, c->stream));
    *n_out = kept;
    return TWOSD_OK;
}

}  // namespace

extern "C" int twosd_fray_key(const double *ray, int mv, uint64_t *key, double *normalised) {
    if (!ray || mv <= 0) return fail(TWOSD_E_ARG, "fray_key: bad arguments");
    std::vector<double> t(ray, ray + mv);
    fr::snap(t.data(), mv, kRayZero);
    if (!fr::normalise(t.data(), mv, t.data())) return fail(TWOSD_E_ARG, "fray_key: the ray is all zero or not finite");
    if (key) *key = fr::key(t.data(), mv);
    if (normalised) std::copy(t.begin(), t.end(), normalised);
    return TWOSD_OK;
}

extern "C" int twosd_fray_push(twosd_ctx *c, int count, const double *rays, int *out_index, int *new_size) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "fray_push: no template");
    if (count < 0 || (count > 0 && !rays)) return fail(TWOSD_E_ARG, "fray_push: bad arguments");
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = fray_init(c))) return rc;
    FrayState &S = c->fray;
    if (count > 0) {
        if ((rc = S.in.fit((size_t)count * S.mv)) || (rc = S.idx.fit(count))) return rc;
        HIPCHK(hipMemcpy(S.in, rays, sizeof(double) * count * S.mv, hipMemcpyHostToDevice));
        if ((rc = fray_push_device(c, count, S.in, S.idx))) return rc;
        if (out_index) HIPCHK(hipMemcpy(out_index, S.idx, sizeof(int) * count, hipMemcpyDeviceToHost));
    }
    if (new_size) *new_size = S.size;
    return TWOSD_OK;
}

extern "C" int twosd_fray_size(twosd_ctx *c, int *size) {
    if (!c || !size) return fail(TWOSD_E_ARG, "fray_size: NULL");
    *size = c->fray.size;
    return TWOSD_OK;
}

extern "C" int twosd_fray_get(twosd_ctx *c, int first, int count, double *out) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "fray_get: no template");
    if (first < 0 || count < 0 || first + count > c->fray.size || (count > 0 && !out))
        return fail(TWOSD_E_ARG, "fray_get: range [%d,%d) outside %d rays", first, first + count, c->fray.size);
    if (count == 0) return TWOSD_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, c->fray.F + (size_t)first * c->fray.mv, sizeof(double) * count * c->fray.mv, hipMemcpyDeviceToHost));
    return TWOSD_OK;
}

extern "C" int twosd_fray_clear(twosd_ctx *c) {
    if (!c) return fail(TWOSD_E_ARG, "fray_clear: NULL");
    if (c->fray.d_meta) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipMemset(c->fray.d_meta, 0, sizeof(int) * 3));
    }
    c->fray.size = 0;
    return TWOSD_OK;
}

extern "C" int twosd_solve_rays(twosd_ctx *c, int epi, const double *x, int first, int count, int cap, int push,
                                int *n_infeasible, int *n_rays, int *scen, double *rays, int *row, int *head, int *status) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "solve_rays: no template");
    if (!c->bp.has_basis) return fail(TWOSD_E_STATE, "solve_rays: no warm-start basis (twosd_compute_basis / twosd_set_basis)");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "solve_rays: epigraph %d does not exist", epi);
    const EpiDevice &E = c->epis[epi];
    if (first < 0 || count < 0 || first + count > E.count)
        return fail(TWOSD_E_ARG, "solve_rays: range [%d,%d) outside %d scenarios", first, first + count, E.count);
    if (cap < 0 || !n_infeasible || !n_rays || (cap > 0 && !scen) || (c->n1 > 0 && !x))
        return fail(TWOSD_E_ARG, "solve_rays: cap >= 0, n_infeasible, n_rays, scen and x required");
    *n_infeasible = 0;
    *n_rays = 0;
    if (count == 0) return TWOSD_OK;
    HIPCHK(hipSetDevice(c->device));
    const int m = c->L.m;
    const double *d_dv = E.d_dv + (size_t)first * c->k;
    int rc = run_lp(c, x, d_dv, count, LpRun());
    if (rc) return rc;
    // the batch's statistics as twosd_solve_batch keeps them; that some LP is not optimal is what
    // the caller asked about, and which kind is decided below
    rc = copy_lp_outputs(c, count, nullptr, nullptr, nullptr, status, E.d_w + first);
    if (rc && rc != TWOSD_E_LP) return rc;
    if (rc == TWOSD_OK) return TWOSD_OK;   // every scenario optimal
    // the infeasible scenarios, ascending
    FrayState &S = c->fray;
    if ((rc = S.flag.fit((size_t)count)) || (rc = S.list.fit((size_t)count)) || (rc = S.cnt.fit(2))) return rc;
    size_t need = 0;
    HIPCHK(hipcub::DeviceSelect::Flagged(nullptr, need, hipcub::CountingInputIterator<int>(0), S.flag.p, S.list.p, S.cnt.p + 1, count,
                                         c->stream));
    if ((rc = S.tmp.fit(need))) return rc;
    HIPCHK(hipMemsetAsync(S.cnt, 0, sizeof(int) * 2, c->stream));
    hipLaunchKernelGGL(ray_flag_kernel, dim3(std::max(1, std::min(4096, (count + 255) / 256))), dim3(256), 0, c->stream, count,
                       c->d_status.p, S.flag.p, S.cnt.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipcub::DeviceSelect::Flagged(S.tmp.p, need, hipcub::CountingInputIterator<int>(0), S.flag.p, S.list.p, S.cnt.p + 1, count,
                                         c->stream));
    int cnt[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(cnt, S.cnt, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int nI = cnt[1];
    *n_infeasible = nI;
    if (cnt[0]) return fail(TWOSD_E_LP, "solve_rays: %d of %d scenario LPs ended at the iteration limit or numerically (see status[])", cnt[0], count);
    if (nI == 0 || cap == 0) return TWOSD_OK;
    if ((rc = S.ray_out.fit((size_t)cap * m)) || (rc = S.row_out.fit(cap)) || (rc = S.scen_out.fit(cap)) ||
        (rc = S.sel.fit(kRayChunk)) || (rc = S.zero.fit(kRayChunk)) || (head && (rc = S.head_out.fit((size_t)cap * m))))
        return rc;
    HIPCHK(hipMemsetAsync(S.zero, 0, sizeof(int) * kRayChunk, c->stream));   // "optimal" for every list position: all count
    // re-solve in chunks from the recorded pool picks with the RAY instantiation; of each chunk the
    // first occurrence of every ray key not seen in an earlier chunk is kept, until cap rays
    std::unordered_set<unsigned long long> seen;
    std::vector<int> reps, rrow, sel;
    std::vector<unsigned long long> keys;
    int nr = 0;
    int nrem = nI;   // the list still to re-solve is S.list[p0, p0 + nrem)
    S.resolved = S.filtered = 0;
    for (int p0 = 0; nrem > 0 && nr < cap;) {
        // a scenario that a ray already held or found cuts off at x needs no ray of its own: the
        // row of that ray will cover it.  (The rays found so far are in F when push != 0.)
        if (c->k <= 127 && (p0 > 0 || S.size > 0)) {
            int kept = nrem;
            if (S.size > 0 && (rc = filter_list(c, x, S.F, S.size, d_dv, p0, nrem, &kept))) return rc;
            if (!push && nr > 0 && kept > 0 && (rc = filter_list(c, x, S.ray_out, nr, d_dv, p0, kept, &kept))) return rc;
            S.filtered += nrem - kept;
            nrem = kept;
            if (nrem == 0) break;
        }
        const int nc = std::min(kRayChunk, nrem);
        S.resolved += nc;
        LpRun r;
        r.want_ray = true;
        r.want_head = head != nullptr;
        r.d_list = S.list + p0;
        r.nlist = nc;
        double us = 0.0;
        r.lp_us_out = &us;
        if ((rc = run_lp(c, x, d_dv, count, r))) return rc;
        c->last.lp_us += us;   // LP kernel time of the call: main pass + re-solves
        const int *d_reps = nullptr;
        int U = 0;
        if ((rc = vkey_first_occurrences(c, nc, S.ray_key, S.zero, &d_reps, &U))) return rc;
        reps.resize(U); keys.resize(nc); rrow.resize(nc);
        HIPCHK(hipMemcpy(reps.data(), d_reps, sizeof(int) * U, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(keys.data(), S.ray_key, sizeof(unsigned long long) * nc, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(rrow.data(), S.ray_row, sizeof(int) * nc, hipMemcpyDeviceToHost));
        int lost = 0;
        for (int i = 0; i < nc; ++i) lost += rrow[i] < 0;
        if (lost) return fail(TWOSD_E_LP, "solve_rays: %d of %d re-solved scenarios did not end infeasible again", lost, nc);
        sel.clear();
        for (int u = 0; u < U && nr + (int)sel.size() < cap; ++u)
            if (seen.insert(keys[reps[u]]).second) sel.push_back(reps[u]);
        const int ns = (int)sel.size();
        const int pc = p0;
        p0 += nc;
        nrem -= nc;
        if (ns == 0) continue;
        HIPCHK(hipMemcpy(S.sel, sel.data(), sizeof(int) * ns, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(ray_gather_kernel, dim3((unsigned)std::min<size_t>(1024, ((size_t)ns * m + 255) / 256)), dim3(256), 0, c->stream,
                           ns, m, nr, first, S.sel.p, S.list.p + pc, S.ray.p, S.ray_row.p, head ? c->d_head_out.p : nullptr, S.ray_out.p,
                           S.row_out.p, head ? S.head_out.p : nullptr, S.scen_out.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));   // S.sel and the re-solve's outputs are free again
        if (push && (rc = fray_push_device(c, ns, S.ray_out + (size_t)nr * m, nullptr))) return rc;
        nr += ns;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    *n_rays = nr;
    if (nr == 0) return TWOSD_OK;
    HIPCHK(hipMemcpy(scen, S.scen_out, sizeof(int) * nr, hipMemcpyDeviceToHost));
    if (rays) HIPCHK(hipMemcpy(rays, S.ray_out, sizeof(double) * nr * m, hipMemcpyDeviceToHost));
    if (row) HIPCHK(hipMemcpy(row, S.row_out, sizeof(int) * nr, hipMemcpyDeviceToHost));
    if (head) HIPCHK(hipMemcpy(head, S.head_out, sizeof(int) * nr * m, hipMemcpyDeviceToHost));
    return TWOSD_OK;
}

extern "C" int twosd_last_ray_stats(twosd_ctx *c, int64_t *resolved, int64_t *filtered, double *scan_us) {
    if (!c) return fail(TWOSD_E_ARG, "last_ray_stats: NULL");
    if (resolved) *resolved = c->fray.resolved;
    if (filtered) *filtered = c->fray.filtered;
    if (scan_us) *scan_us = c->fray.scan_us;
    return TWOSD_OK;
}

extern "C" int twosd_feas_scan(twosd_ctx *c, int epi, const double *x, int first, int count, double *ray_max, int *ray_arg,
                               double *alpha, double *beta, int64_t *n_cut_off, unsigned char *cut_off) {
    if (!c || !c->has_template) return fail(TWOSD_E_STATE, "feas_scan: no template");
    if (epi < 0 || epi >= (int)c->epis.size()) return fail(TWOSD_E_ARG, "feas_scan: epigraph %d does not exist", epi);
    const EpiDevice &E = c->epis[epi];
    if (first < 0 || count <= 0 || first + count > E.count)
        return fail(TWOSD_E_ARG, "feas_scan: range [%d,%d) outside %d scenarios (at least one)", first, first + count, E.count);
    if (c->n1 > 0 && !x) return fail(TWOSD_E_ARG, "feas_scan: x is NULL");
    FrayState &S = c->fray;
    const int J = S.size, m = c->L.m, k = c->k, n1 = c->n1;
    if (J == 0) return fail(TWOSD_E_STATE, "feas_scan: the ray set is empty");
    if (k > 127) return fail(TWOSD_E_UNSUPPORTED, "feas_scan: k = %d random elements exceeds the cut kernel envelope (127)", k);
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = feas_scan_device(c, x, S.F, J, E.d_dv + (size_t)first * k, nullptr, count, first))) return rc;
    std::vector<double> rmax(J);
    std::vector<int> rarg(J);
    unsigned long long ncut = 0;
    HIPCHK(hipMemcpyAsync(rmax.data(), S.rmax, sizeof(double) * J, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(rarg.data(), S.rarg, sizeof(int) * J, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&ncut, S.ncut, sizeof(ncut), hipMemcpyDeviceToHost, c->stream));
    if (cut_off) HIPCHK(hipMemcpyAsync(cut_off, S.cut, (size_t)count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[EV_MARK_0], c->ev[EV_MARK_1]);
    S.scan_us = 1e3 * ms;
    if (ray_max) std::copy(rmax.begin(), rmax.end(), ray_max);
    if (ray_arg) std::copy(rarg.begin(), rarg.end(), ray_arg);
    if (n_cut_off) *n_cut_off = (int64_t)ncut;
    if (alpha || beta) {
        // the row of (ray j, its worst scenario): that scenario's right-hand side and T (the template's
        // with its element values), then feas_rays.h's row
        std::vector<double> F((size_t)J * m), dv((size_t)J * std::max(k, 1)), rb(m), T, bj(std::max(n1, 1));
        HIPCHK(hipMemcpy(F.data(), S.F, sizeof(double) * J * m, hipMemcpyDeviceToHost));
        for (int j = 0; j < J && k > 0; ++j)
            HIPCHK(hipMemcpy(dv.data() + (size_t)j * k, E.d_dv + (size_t)rarg[j] * k, sizeof(double) * k, hipMemcpyDeviceToHost));
        for (int j = 0; j < J; ++j) {
            rb = c->r;
            T = c->T;
            for (int e = 0; e < k; ++e) {
                const double d = dv[(size_t)j * k + e];
                if (c->pos_col[e] < 0) rb[c->pos_row[e]] += d;
                else T[(size_t)c->pos_row[e] * n1 + c->pos_col[e]] += d;
            }
            double a = 0.0;
            fr::row(F.data() + (size_t)j * m, m, rb.data(), T.data(), n1, &a, bj.data());
            if (alpha) alpha[j] = a;
            if (beta) std::copy(bj.begin(), bj.begin() + n1, beta + (size_t)j * n1);
        }
    }
    return TWOSD_OK;
}
