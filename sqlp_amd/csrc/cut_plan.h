// cut_plan.h -- the launch plan of one cut as a pure function of its shape and the environment
// knobs: the passes, the persistent grid and its tail split, the block counts of every stage, the
// partial-sum slot layout and the sizes of the buffers that follow from them.  No HIP in here: the
// driver (cut_kernel.hip) reads the plan, and tests/native/cut_plan_check.cpp includes this file
// alone and prints plans on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace twosd {
#pragma GCC visibility push(hidden)

constexpr int kHistLds = 256;      // |V| up to this: the block histogram lives in LDS
constexpr int kCandC = 16;         // logged candidates per (scenario, lane group); count kCandC + 1 = overflow
static_assert(4 * kCandC == 64, "one 64-lane step of the fixup's enumeration covers one scenario's log slots");
constexpr int kVT2 = 32;                 // vertices per LDS chunk (two 16-vertex MFMA tiles)
constexpr int kCutTile2 = 128;           // scenarios per block tile (4 waves x 2 x 16)
// k-rows staged per chunk of the fp32 pass: KB k-blocks of 4, rounded up to whole 8-row (1 KiB) DMA instructions
constexpr int kr32(int KB) { return 8 * ((KB + 1) / 2); }

// The environment knobs of a cut (A/B and test hooks), defaults as with nothing set.
struct CutKnobs {
    // read once per process (function-local statics of cut_knobs)
    int bpc = 0;                     // TWOSD_CUT_BPC: argmax blocks per CU (<= 0: the resident occupancy)
    int fix_per_cu = 3;              // TWOSD_FIX_BPC: fixup blocks per CU
    int hist_lds_max = kHistLds;     // TWOSD_HIST_LDS: |V| up to which the block histogram lives in LDS
    // read on every cut (tests set these between cuts of one process)
    bool f32 = true;                 // TWOSD_CUT_F32=0: no reduced-precision pass
    bool i8 = true;                  // TWOSD_CUT_I8=0: the fp32 pass instead of the integer one
    bool tail_split = true;          // TWOSD_CUT_TAIL=0: whole tiles only
    bool twins = true;               // TWOSD_CUT_TWINS=0: dominated twins stay in the argmax (the same picks; more re-decided rows)
    size_t log_max = UINT32_MAX;     // TWOSD_CUT_LOG_MAX: candidate-log slots a cut may need (test hook)
};

inline bool cut_knob_on(const char *name) { return !getenv(name) || atoi(getenv(name)) != 0; }

inline CutKnobs cut_knobs() {
    static const int bpc_env = getenv("TWOSD_CUT_BPC") ? atoi(getenv("TWOSD_CUT_BPC")) : 0;
    static const int fix_per_cu = getenv("TWOSD_FIX_BPC") ? std::max(1, atoi(getenv("TWOSD_FIX_BPC"))) : 3;
    static const int hist_lds_max = getenv("TWOSD_HIST_LDS") ? atoi(getenv("TWOSD_HIST_LDS")) : kHistLds;
    CutKnobs kn;
    kn.bpc = bpc_env;
    kn.fix_per_cu = fix_per_cu;
    kn.hist_lds_max = hist_lds_max;
    kn.f32 = cut_knob_on("TWOSD_CUT_F32");
    kn.i8 = cut_knob_on("TWOSD_CUT_I8");
    kn.tail_split = cut_knob_on("TWOSD_CUT_TAIL");
    kn.twins = cut_knob_on("TWOSD_CUT_TWINS");
    if (const char *e = getenv("TWOSD_CUT_LOG_MAX")) kn.log_max = (size_t)atoll(e);
    return kn;
}

struct CutShape {
    int N, nv, k;      // scenarios, vertices, random elements
    int num_cus;
    int bpc;           // resident argmax blocks per CU as found (cut_argmax_bpc: the occupancy query is HIP)
};

struct CutPlan {
    // the passes: k4 = k padded to 4; KB / KB32 the k-block instantiations of the fp64 pass (k element
    // rows plus the vertex base row) and of the reduced-precision passes (element rows only); KS8 the
    // integer pass's 64-wide k-steps
    int k4, KB, KB32, KS8;
    bool want32, wanti8;
    // the persistent argmax grid: units [0, full) are whole scenario tiles, the tiles past them are
    // cut into S vertex ranges each
    int ntiles, nchunks, full, S, nunits, nblocks;
    // the fixup (fx_gs: whole-tile scenarios per wave step), tail merge and rescan
    int fx_gs, fix_blocks, ntail, merge_blocks, resc_blocks;
    // partial-sum slots, four per block, in the order argmax [0, slot_fix), fixup, tail merge, rescan
    int slot_fix, slot_merge, slot_rescan;
    size_t slots;
    size_t cand_need, tcand_need;    // candidate-log slots of the whole tiles / the tail ranges
    int hist_lds;                    // 1: per-block LDS histogram
    int vcap32, rows, rows32;        // PKTc's row stride, its rows and PKTc32's
    double band_scale, band_scale32;
};

// the instantiation for k4 chunk rows out of the ascending table kbs (-1: past the envelope)
inline int cut_kb_for(const int *kbs, int nkb, int k4) {
    for (int i = 0; i < nkb; ++i)
        if (4 * kbs[i] >= k4) return kbs[i];
    return -1;
}

// the passes of a cut over k elements; false: k past the envelope
inline bool cut_plan_passes(int k, const CutKnobs &kn, const int *kbs, int nkb, CutPlan &pl) {
    pl.k4 = (std::max(k, 1) + 3) & ~3;
    // the chunk's k-rows: k element rows plus the vertex base row
    pl.KB = cut_kb_for(kbs, nkb, (k + 1 + 3) & ~3);
    if (pl.KB < 0) return false;
    // the MFMA pass in fp32 (cut_argmax3_kernel, the element rows only: no base row) unless
    // TWOSD_CUT_F32=0; a cut whose operands leave the fp32 range runs the fp64 pass anyway (decided
    // on the device, cut_band_select_kernel)
    pl.KB32 = cut_kb_for(kbs, nkb, pl.k4);
    pl.want32 = pl.KB32 > 0 && kn.f32;
    // the integer (int8-limb) MFMA pass in place of the fp32 one (cut_argmax4_kernel; k <= 128 holds
    // for every k the envelope admits) unless TWOSD_CUT_I8=0; the device falls back to the fp32 or
    // fp64 pass for a cut it does not fit (cut_band_select_kernel)
    pl.wanti8 = pl.want32 && kn.i8;
    pl.KS8 = pl.KB32 <= 16 ? 1 : 2;
    return true;
}

enum CutPlanStatus { CUT_PLAN_OK = 0, CUT_PLAN_K_ENVELOPE, CUT_PLAN_LOG_SLOTS };

inline CutPlanStatus cut_plan(const CutShape &sh, const CutKnobs &kn, const int *kbs, int nkb, CutPlan &pl) {
    const int N = sh.N, nv = sh.nv, k = sh.k;
    if (!cut_plan_passes(k, kn, kbs, nkb, pl)) return CUT_PLAN_K_ENVELOPE;
    pl.ntiles = (N + kCutTile2 - 1) / kCutTile2;
    pl.nchunks = (nv + kVT2 - 1) / kVT2;
    // The persistent grid runs whole tiles round after round; the tiles past the last full
    // round are cut into S vertex ranges (at least 4 chunks each) so that the last round is as
    // full as the others.  S minimises the tail's length ceil(T S / B) / S in tile durations.
    const int B = sh.bpc * sh.num_cus;
    pl.full = pl.ntiles;
    pl.S = 1;
    if (kn.tail_split && pl.nchunks >= 8) {
        const int T = pl.ntiles % B;
        double best = 1.0;
        for (int s_ = 2; T > 0 && s_ <= std::min(64, pl.nchunks / 4); ++s_) {
            const double cost = (double)(((long long)T * s_ + B - 1) / B) / s_;
            if (cost < best - 1e-9) { best = cost; pl.S = s_; }
        }
        if (pl.S > 1) pl.full = pl.ntiles - T;
    }
    pl.nunits = pl.full + (pl.ntiles - pl.full) * pl.S;
    pl.nblocks = std::max(1, std::min(pl.nunits, B));
    // the fixup takes 64 scenarios per wave step: enough waves that every SIMD holds several; 3 blocks
    // per CU = its resident occupancy (launch bounds, LDS), so no block waits for a second round
    // (storm 1M at x_EV: 0.88 ms at 4, 0.69 at 3, 0.86 at 2, 0.82 at 8: profiles/r06/ab_fixup_grid.txt).
    // Scenarios per wave step: 64, or 32 / 16 when 64 would leave fewer waves than 3 resident blocks
    // per CU hold (a 125k shard at N = 8: 1953 waves of one step each, every flagged row's batch
    // latency in series)
    pl.fx_gs = 64;
    while (pl.fx_gs > 16 && (long long)(N + pl.fx_gs - 1) / pl.fx_gs < 12ll * sh.num_cus) pl.fx_gs /= 2;
    pl.fix_blocks = std::max(1, std::min((N + 4 * pl.fx_gs - 1) / (4 * pl.fx_gs), kn.fix_per_cu * sh.num_cus));
    pl.ntail = pl.S > 1 ? N - pl.full * kCutTile2 : 0;
    pl.merge_blocks = pl.ntail > 0 ? std::max(1, std::min((pl.ntail + 3) / 4, sh.num_cus)) : 0;
    pl.resc_blocks = std::max(1, std::min((N + 255) / 256, sh.num_cus));
    pl.slot_fix = pl.nblocks * 4;
    pl.slot_merge = pl.nblocks * 4 + pl.fix_blocks * 4;
    pl.slot_rescan = pl.nblocks * 4 + pl.fix_blocks * 4 + pl.merge_blocks * 4;
    pl.slots = (size_t)pl.nblocks * 4 + (size_t)pl.fix_blocks * 4 + (size_t)pl.merge_blocks * 4 + (size_t)pl.resc_blocks * 4;
    // candidate logs: rows padded to whole tiles (the padding scenarios of a tile log too)
    pl.cand_need = (size_t)pl.full * kCutTile2 * 4 * kCandC;
    pl.tcand_need = (size_t)(pl.ntiles - pl.full) * kCutTile2 * pl.S * 4 * kCandC;
    pl.hist_lds = nv <= kn.hist_lds_max ? 1 : 0;
    pl.vcap32 = (nv + 31) & ~31;
    pl.rows = 4 * pl.KB;
    pl.rows32 = pl.want32 ? kr32(pl.KB32) : 0;
    // band: the MFMA score and the restated one both add base[v] to a (k + 1)-term dot and differ
    // by at most 2 gamma_{k+4} (|base[v]| + sum_e |PK coef dv|) (one more rounding per T element
    // term, coef folded on the other side); twice that for safety
    const double u = ldexp(1.0, -53), u32 = ldexp(1.0, -24), nk = (double)(k + 4);
    pl.band_scale = 2.0 * 2.0 * (nk * u / (1.0 - nk * u));
    pl.band_scale32 = 2.0 * 2.0 * (nk * u32 / (1.0 - nk * u32));
    // the argmax forms log offsets as 32-bit indices (log0 / lstep): past 2^32 slots (~67M
    // scenarios in one epigraph) they would wrap and the fixup would read slots no kernel wrote
    if (pl.cand_need > kn.log_max || pl.tcand_need > kn.log_max) return CUT_PLAN_LOG_SLOTS;
    return CUT_PLAN_OK;
}

#pragma GCC visibility pop
}  // namespace twosd
