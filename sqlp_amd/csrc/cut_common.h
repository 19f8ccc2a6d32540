// cut_common.h -- what the cut's translation units share (cut_kernel.hip: the driver; cut_prep.hip,
// cut_argmax.hip, cut_fixup.hip: the stages): the kernels' parameter block, the constants and
// device helpers more than one stage uses, the named slots of the two diagnostic arrays, the
// workspace, and the stage functions.  Every kernel is launched only from the file that defines it.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "twosd_ctx.h"
#include "cut_i8.h"
#include "cut_plan.h"

namespace twosd {

constexpr double kFix = 4611686018427387904.0;   // 2^62 fixed-point scale of p_w

constexpr int kCandBits = 5;       // bits of one lane group's count in a packed flag (4 groups: 20 bits)

// the k-block counts the three argmax kernels are instantiated for, ascending (22: ssn, k = 86, + base row)
constexpr int kCutKBs[] = {1, 2, 4, 6, 8, 12, 16, 22, 24, 30, 32};
constexpr int kNumKB = sizeof(kCutKBs) / sizeof(kCutKBs[0]);
static_assert(4 * kCutKBs[kNumKB - 1] == 128, "the envelope: at most 128 chunk rows (k <= 127 plus the base row)");

// fstats: the counters of the last cut (twosd_cut_stats)
enum CutStat : int {
    CS_FIX_ROWS = 0,      // scenarios the fixup re-decided
    CS_FIX_CANDS = 1,     // candidates it scored
    CS_FIX_RESCANS = 2,   // rows left to the full re-scan
    CS_FIX_STAMP0 = 3,    // [3, 9): the fixup's phase cycles (-DTWOSD_FIX_STAMPS builds)
    CS_FIX_STAMPS = 6,    // their count
    CS_TWINS = 9,         // dominated twins left out of the argmax (cut_compact_kernel)
    CS_F32_STEPS = 10,    // the fp32 pass's chunk steps, those past the prefilter, lanes past it
    CS_F32_RARE = 11,     //   (-DTWOSD_CUT3_COUNT builds)
    CS_F32_LANES = 12,
    CS_COUNT = 16
};
static_assert(CS_FIX_STAMP0 + CS_FIX_STAMPS == CS_TWINS, "the stamps end where the twin count begins");

// band_bits: the decision bands of the last cut, as bits, and the pass chosen on the device
enum BandSlot : int {
    BAND_F64 = 0,         // the fp64 pass's band
    BAND_F32 = 1,         // the fp32 pass's
    BAND_F32_RANGE = 2,   // != 0: some vertex's operands leave the fp32 range
    BAND_ACTIVE = 3,      // the band of the pass that runs (what every later kernel of the cut reads)
    BAND_PASS = 4,        // that pass: 0 fp64, 1 fp32, 2 integer
    BAND_I8 = 5,          // the integer pass's band
    BAND_COUNT = 8
};

struct CutParams {
    int N, k, k4, nv, vcap, m;
    int hist_lds;          // 1: per-block LDS histogram (nv <= kHistLds), flushed once per block
    double tie_rel, inv_total;
    const double *dv;      // N x k
    const double *w;       // N
    const double *coef;    // k4 (zero padded)
    const double *PK;      // nv x k4
    const double *PKT;     // k4 x vcap
    const double *PKO;     // nv x k4: PK with its columns in the restated order (PKO[v][q] = PK[v][eord[q]])
    const double *PKTc;    // 4 KB x vcap32: coef_e(x) * PKT over the argmax's vertices, zero padded (cut_argmax2_kernel's LDS-DMA source)
    int vcap32;            // row stride of PKTc (a multiple of 32 >= nv)
    const int *vmap;       // the argmax's vertices (dominated twins left out), ascending: column c of PKTc is vertex vmap[c]
    const int *nvc;        // their count (device: set per x by cut_compact_kernel)
    const double *PKOc;    // PKO rows of the argmax's vertices (row c: vertex vmap[c]), per x
    const double *basec;   // base of the argmax's vertices, per x (vcap32 entries; past nvc unused)
    const double *base;    // nv: pi_v . bvec in index order (the restatement's base dot)
    const int *eord;       // k: elements by ascending row (the restated score's order)
    const unsigned long long *band_bits;   // the ACTIVE band of this cut, as bits (cut_band_select_kernel)
    const unsigned long long *mode;        // this cut's MFMA pass: 2 integer limbs (cut_argmax4_kernel), 1 fp32 (cut_argmax3_kernel), 0 fp64 (cut_argmax2_kernel)
    const float *basec32;  // vcap32: basec rounded up to fp32 (-inf past nvc): the fp32 pass's prefilter
    const int8_t *PKq;     // the integer pass's chunk source: per 32-vertex chunk, limb, 64-wide k-step the int8 limb plane (cut_pkq_kernel)
    const float *scq;      // vcap32: the integer pass's output scale 2^(S_v + kOutShift) per compacted vertex (0 past nvc)
    const double *dsc;     // 128: the deltas' quantisation factors 2^(kQ - E_e) (0 past k)
    const float *PKTc32;   // KR32 x vcap32: PKTc's element rows rounded to fp32, no base row (cut_argmax3_kernel's LDS-DMA source)
    double band_scale;     // 4 gamma_{k+4}: twice the 2 gamma bound
    int *arg; double *val; int *flag;   // N; flag != 0: re-decide (main rows: 4-bit log counts per lane group)
    int *cand;             // candidate logs of the whole tiles: [(s * 4 + g) * kCandC + i]
    unsigned long long *fstats;   // the cut's counters (CutStat)
    int *tcand;            // of the tail ranges: [(((s - t0) * tail_S + range) * 4 + g) * kCandC + i]
    unsigned long long *hist;           // nv (fixed point)
    unsigned long long *hist_part;      // gridDim.x x nv block histograms (hist_lds mode)
    double *partial;       // slots x (k + 1): [sum p*val, S_0..S_{k-1}]
    // work units of cut_argmax2_kernel: units [0, full_units) are whole scenario tiles; the
    // tiles past them (the last, partial round of the persistent grid) are cut into tail_S
    // vertex ranges each, and such a unit leaves its per-scenario (M, I, log counts) in tp_* at
    // [(s - 128 full_units) tail_S + range] for cut_tail_merge_kernel
    int full_units, tail_S;
    int fx_gs;             // cut_fixup_kernel: whole-tile scenarios per wave step (64; 32 / 16 for small batches)
    double *tp_m;
    int *tp_i, *tp_f;
};

// the decision band of this cut (written by cut_vbase_kernel) through the scalar cache: a
// wave-uniform value held in SGPRs rather than a VGPR pair (the 3-blocks-per-CU argmax would
// spill it)
__device__ __forceinline__ double cut_band_scalar(const CutParams &P) {
    return __longlong_as_double((long long)((const __attribute__((address_space(4))) unsigned long long *)P.band_bits)[0]);
}

// floor of the decision band around a running maximum M: a vertex below it cannot be the
// restatement's pick (monotone in M for tie_rel < 1)
__device__ __forceinline__ double band_floor(double M, double rel, double band) { return M - (rel * (1.0 + fabs(M)) + band); }

typedef int i4 __attribute__((ext_vector_type(4)));

// The image of one 32-vertex chunk of the integer pass, in global memory and (copied lane-linearly
// by the LDS-DMA) in LDS: [limb][k-step][g][vertex 0..31][16 bytes]; byte b of (k-step ks, g) is element
// e = 64 ks + 16 g + b, the 16 k-values lane (g, j) feeds one MFMA.  A wave's ds_read_b128 of a
// fragment reads 16 consecutive bytes per lane, 256 contiguous bytes per 16 lanes of a g:
// conflict-free.
__host__ __device__ constexpr int i8_chunk_bytes(int KS) { return ci8::kL * KS * 2048; }
__host__ __device__ constexpr int i8_frag_off(int KS, int l, int ks, int g, int vv) { return ((l * KS + ks) * 4 + g) * 512 + vv * 16; }

template <typename T>
using CutBuf = DevBuf<T, 4>;
struct CutWs {
    CutBuf<double> PK, PKT, PKO;
    CutBuf<double> PKTc;
    CutBuf<float> PKTc32;               // the fp32 pass's chunk source
    CutBuf<float> basec32;              // the fp32 and integer passes' prefilter bases
    CutBuf<int8_t> PKq;                 // the integer pass's chunk images (limb planes), per x
    CutBuf<float> scq;                  // its output scales per compacted vertex, per x
    CutBuf<double> dsc;                 // its delta quantisation factors (128)
    int i8_ks = 0;                      // k-steps of the images the last cut wrote (0: none)
    // PK rows up to date, the vertices PK / PKT / PKO / phash / tprev hold, and their row length
    int pk_count = 0, pk_vcap = 0, pk_k4 = 0;
    CutBuf<int> rows;
    CutBuf<int> eord;    // elements by ascending row: the order of the restated score's dot
    CutBuf<unsigned long long> phash;   // per vertex: hash of its PK row (bits)
    CutBuf<int> tprev;                  // per vertex: previous vertex with a bit-identical PK row, or -1
    CutBuf<unsigned long long> tw_hs;   // twin rebuild by sort: sorted hashes, vertex ids in / out, cub scratch
    CutBuf<int> tw_vin, tw_vout;
    CutBuf<char> tw_tmp;
    CutBuf<int> vmap, nvc;   // per x: the argmax's vertices and their count
    CutBuf<double> PKOc, basec;   // per x: their PKO rows and bases (vmap order)
    CutBuf<double> coef, bvec, base, partial, sums;
    CutBuf<double> gpart, g;
    CutBuf<int> arg, flag;
    CutBuf<double> val;
    CutBuf<unsigned long long> hist, hist_part;
    CutBuf<double> part2;
    CutBuf<double> tp_m;
    CutBuf<int> tp_i, tp_f;
    CutBuf<int> cand, tcand;    // candidate logs (whole tiles / tail ranges)
    CutBuf<unsigned long long> fstats;     // counters of the last cut (CutStat)
    CutBuf<unsigned long long> band_bits;  // bands and pass of the last cut (BandSlot)
    // per epigraph: max |dv[., e]| over its scenarios (bits), the rows folded in so far
    std::vector<CutBuf<unsigned long long>> dmax;
    std::vector<int> dmax_rows, dmax_k;
    int m = 0, vec_m = 0;
    std::vector<double> h_coef, h_bvec;   // pinned-lifetime host staging for async uploads
};

inline CutWs *cws(twosd_ctx *c) {
    if (!c->cut_ws) c->cut_ws.reset(new CutWs());
    return c->cut_ws.get();
}

// ---- the stages, each in the file of its kernels.  The *_stage functions only enqueue on the
// stream (every buffer is sized by the driver before the first one); the driver checks
// hipGetLastError once after the last.
#pragma GCC visibility push(hidden)
// cut_prep.hip
int update_pk(twosd_ctx *c);   // bring PK / PKT / PKO and the twin links up to date with the vertex set
// the epigraph's max |dv| per element, folded in for the rows added since the last cut
int cut_fold_dmax(twosd_ctx *c, int epi, int N, int k);
// the operands of a cut at x: vertex bases and bands, the pass, the argmax's vertex list and its
// chunk sources
void cut_operand_stage(twosd_ctx *c, int epi, const CutShape &sh, const CutPlan &pl, bool twins);
// The same operands for feasibility rays (feas.hip): a ray is structurally a dual vertex.  For the J
// rays F (J x m, device) at x: their element gathers PK / PKT / PKO (J x k4, k4 x J, J x k4) by
// cut_pk_kernel and their bases sigma_j . (r - T x) by cut_vbase_kernel, with coef_e(x) and r - T x
// uploaded into the cut's own vectors.  scratch: k + 1 + BAND_COUNT words (the band the base kernel
// folds is not used).  *coef / *eord / *k4: the cut's coef_e(x) table, element order and row length.
int cut_ray_operands(twosd_ctx *c, const double *x, int J, const double *d_F, double *PK, double *PKT, double *PKO, double *base,
                     unsigned long long *scratch, const double **coef, const int **eord, int *k4);
// cut_kernel.hip
void host_bvec_coef(const twosd_ctx *c, const double *x, int k4, std::vector<double> &bvec, std::vector<double> &coef);
int cut_size_vectors(CutWs *w, int m);
// cut_argmax.hip
int cut_argmax_bpc(int k, const CutKnobs &kn);   // CutShape::bpc: the knob, else the pass's resident blocks per CU
void cut_argmax_stage(const CutPlan &pl, const CutParams &P, hipStream_t s);   // the passes and the histogram reduce
void cut_scores_stage(const CutPlan &pl, const CutParams &P, int KS, float *d_out, hipStream_t s);   // debug scores of the integer pass
// cut_fixup.hip
void cut_fixup_stage(const CutPlan &pl, const CutParams &P, hipStream_t s);    // tail merge, fixup, rescan
#pragma GCC visibility pop

}  // namespace twosd
