// twosd_ctx.h -- the opaque twosd_ctx behind the C ABI (library-internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <memory>
#include <thread>
#include <vector>
#include "devbuf.h"
#include "twosd_internal.h"
#include "basis_pool.h"

// a failed HIP call ends the enclosing function with TWOSD_E_DEVICE and the call's text
#define HIPCHK(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return twosd::fail(TWOSD_E_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

namespace twosd {

// the pinned staging slots (twosd_ctx::stage) by use; a slot's buffer grows to its largest use
enum StageSlot : int {
    STG_POOL_RCOL = 0, STG_POOL_CROW, STG_POOL_RVAL, STG_POOL_CVAL, STG_POOL_D0,   // upload_pool: B^{-1} CSR / CSC, d0
    STG_ELEM_KE, STG_ELEM_KIX, STG_ELEM_KRAW, STG_ELEM_KV,                         // prepare_elements: CSR and ELL rows
    STG_PG_TOT,       // source table read-back: tot (4 nsrc) [, nztot (nsrc): the gathered table's], valid (nsrc)
    STG_FREE_10,      // unused
    STG_PG_NZ,        // pg_compute: nztot of the first FTRAN pass
    STG_PG_IOFF,      // intermediate CSC offsets before their upload
    STG_RT_SEG,       // copy-segment list of rt_copy
    STG_RT_HDR,       // pack header
    STG_CAND,         // candidate lists of the two-level selection
    STG_COUNT
};
static_assert(STG_PG_TOT == 9 && STG_CAND == 15 && STG_COUNT == 16, "a slot keeps its buffer: do not renumber");

// the training range a cached box of the deltas was taken over (epigraph, first, count, and the
// epigraph's size then); the default matches no range
struct BoxCache {
    int epi = -1, first = -1, count = -1, n = -1;
    bool operator==(const BoxCache &o) const { return epi == o.epi && first == o.first && count == o.count && n == o.n; }
};

struct EpiDevice {
    DevBuf<double> d_dv;          // count x k scenario deltas (value - template value)
    DevBuf<double> d_w;           // count weights
    int count = 0;
    double total_weight = 0.0;    // epigraph.jl:89, accumulated in insertion order
    std::vector<double> w_host;
};

// stored picks of one cut (twosd_picks_keep): the argmax's vertex index of each of the n scenarios
// the epigraph held then, over the first nv vertices of the set
//
// A tail handle (twosd_tail_keep) lives in the same table: nt >= 0, scen = the nt scenarios of that
// cut scoring above eta in ascending order and d = their nt picks (8 bytes per tail scenario); epi,
// n and nv stay the cut's.  nt < 0: a pick handle.
struct PickSet {
    DevBuf<int> d;                // n picks (a tail handle: nt, by list position)
    DevBuf<int> scen;             // a tail handle's nt scenario indices, ascending
    int epi = -1, n = 0, nv = 0;
    int nt = -1;                  // tail handle: the list's length (0: an empty tail)
    double eta = 0.0;             //   and the eta it was taken at
    bool live = false;
    bool stale = false;           // the vertex set was truncated below nv since: unusable
    bool is_tail() const { return nt >= 0; }
    int entries() const { return nt >= 0 ? nt : n; }   // what a re-formation walks: the list, or the n scenarios
};

// cuts re-formed from stored picks (reform.hip; boot_kernel.hip's bootstrap and risk.hip's tail cut, synchronous on the
// one stream): the pick handles, the template's device copies, and the workspaces and output rows of a call.
// twosd_set_template and twosd_set_random_positions assign a fresh one (every handle dropped).
struct ReformState {
    std::vector<PickSet> picks;
    bool tmpl_ready = false;
    DevBuf<double> d_T, d_r;      // dense T (m x n1), r (m)
    DevBuf<int> d_col;            // k: first-stage column of each random element, -1 for an rhs element
    DevBuf<double> slots, gpart;  // the shards' S partials of one handle; the vertex chunks' g partials
    DevBuf<double> out;           // outputs of a call, rows = (M + 1) x H: [alpha][weight_mark][beta: rows x n1], one copy when small
    double *d_alpha = nullptr, *d_wm = nullptr, *d_beta = nullptr;
    DevBuf<unsigned long long> u64;   // twosd_reform_cuts' own partial buffers (the split's are the caller's)
    DevBuf<double> f64;               //   its S sums; the tail cut's too
    DevBuf<uint8_t> counts;
    double ms[2] = {0, 0};        // device time of the last twosd_reform_cuts: partial sums, finalize (with its copies)
};

// feasibility rays (feas.hip): the ray set F and the workspaces of twosd_solve_rays.  Dropped with
// the template and the random positions, like the pick handles.
struct FrayState {
    int mv = 0, size = 0;         // ray length (the LP's rows), rays in F
    DevBuf<double> F;             // TWOSD_FRAY_MAX x mv normalised rays, insertion order
    DevBuf<unsigned long long> keys;   // their dedup keys (feas_rays.h)
    DevBuf<int> d_meta;           // [0] size, [1] != 0: the last push would have overflowed
    // push: the incoming rays, their normalised forms, keys, validity and resulting indices
    DevBuf<double> in, nrm;
    DevBuf<unsigned long long> inkey;
    DevBuf<int> ok, idx;
    // twosd_solve_rays: the infeasible scenarios (ascending), the re-solve's outputs by list
    // position, the kept rays and what goes with them
    DevBuf<char> flag, tmp;
    DevBuf<int> list, list2, cnt, zero, sel;
    long long resolved = 0, filtered = 0;   // of the last twosd_solve_rays: list positions re-solved / dropped by the scan filter
    DevBuf<double> ray, ray_out;
    DevBuf<int> ray_row, row_out, head_out, scen_out;
    DevBuf<unsigned long long> ray_key;
    // twosd_feas_scan: the rays' operands at x (the cut's prep: element gathers and bases), the
    // blocks' partial maxima, the merged result, the cut-off flags and their count
    DevBuf<double> pk, pkt, pko, base, pmax, rmax, dvsel;
    DevBuf<int> parg, rarg;
    DevBuf<unsigned long long> scratch, ncut;
    DevBuf<unsigned char> cut;
    double scan_us = 0.0;         // device time of the last twosd_feas_scan's scan and merge kernels
};

// risk measures (risk.hip): the workspaces of the quantile selection, the tail cut's own, the
// uploads of twosd_quantile_of_values and the objectives twosd_evaluate_cvar keeps on the device.
// Grow-only scratch: nothing here outlives the call that filled it.
struct RiskState {
    DevBuf<unsigned long long> u64;   // the passes' digit histograms, then the selection record (risk.hip: RiskSel)
    DevBuf<double> part;              // the tail sum's shard partials
    DevBuf<double> val, w;            // quantile_of_values: the caller's values and weights
    DevBuf<int> st;                   //   and statuses
    DevBuf<double> obj;               // evaluate_cvar: the whole range's objectives, overwritten by Y
    DevBuf<int> ost;                  //   and statuses
    DevBuf<unsigned long long> thist; // tail cut: [0] W_t, [1] the total, [2 ..) the per-vertex weights (the rest: ReformState)
    DevBuf<int> tcnt;                 // tail_keep: the 64-scenario tiles' tail counts, then their exclusive offsets and nt
    double ms[2] = {0, 0};            // device time of the last selection / tail re-formation
    double keep_ms = 0.0;             //   and of the last twosd_tail_keep
};

// the slots of twosd_last_timings, in the order the ABI reports them (microseconds)
enum TimeSlot : int {
    T_LP = 0,         // LP kernel of the last batch (solve_push in re-solve mode: main pass + representatives)
    T_DEDUP,          // vertex keys and push of the last solve_push / twosd_dvs_push
    T_CUT_PARTIAL,
    T_CUT_FINALIZE,
    T_POOL_SELECT,    // warm-start selection of the last batch
    T_COUNT
};

// twosd_ctx::ev by owner.  Every call is synchronous on the one stream, so an owner's events are
// free again when its call returns; the push begins after the launch has read its own three.
enum EventSlot : int {
    EV_LP_BEGIN = 0, EV_LP_END = 1, EV_LP_SELECTED = 2,   // the LP launch (run_lp): selection = BEGIN..SELECTED, kernel = SELECTED..END
    EV_PUSH_BEGIN = 2, EV_PUSH_END = 3,                   // the push of solve_push / twosd_dvs_push
    EV_MARK_0 = 4, EV_MARK_1 = 5, EV_MARK_2 = 6,          // up to three marks of one call: cut, bootstrap, solve_push's keys
    EV_COUNT = 8                                          // 7 is free
};

// The last LP batch, as the twosd_last_* getters report it.  The one rule: a non-list launch
// (run_lp) writes N and the two times, its copy_lp_outputs the rest; a list-mode launch never
// touches it (it hands its kernel time to LpRun::lp_us_out).  solve_push adds the
// representatives' re-solve to lp_us and nothing else.
struct LpBatchRecord {
    int N = 0;                           // scenarios of the batch
    double lp_us = 0.0, sel_us = 0.0;    // LP kernel (with its queue records), warm-start selection
    int64_t pivots_sum = 0;
    int pivots_max = 0;
    int64_t ops_sum = 0;                 // executed FMAs
    int64_t eta_entries = 0;
    int64_t retries = 0;                 // pool starts retried from the primary basis
    double obj_wsum = 0.0, obj_w = 0.0;  // sum_s w_s obj_s (fixed-order reduction) and sum_s w_s
};

struct CutWs;    // cut_common.h
struct DvsWs;    // dvs_kernel.hip
struct VkeyWs;   // vkey.hip
void cut_free(CutWs *w);
void dvs_free(DvsWs *w);
void vkey_free(VkeyWs *w);

}  // namespace twosd

// Everything a template re-set clears: twosd_set_template assigns a default-constructed one.
struct TemplateState {
    // pivot sum and size of the last large batch (N >= 4096), the scale of the refresh's auto cap
    // (ranks agree on one cap).  Not part of `last`: it outlives the smaller batches that follow.
    int64_t piv_ref_sum = 0, piv_ref_n = 0;
    int last_train_opt = 0;       // optimal training scenarios of the last refresh
    twosd::LpBatchRecord last;
    double t_us[twosd::T_COUNT] = {};   // T_DEDUP and the cut's two; T_LP / T_POOL_SELECT are last.lp_us / last.sel_us
    // template
    bool has_template = false;
    twosd::HostLP L;              // W CSC, q, sense (host)
    int n1 = 0, R = 0, MP = 0, C = 0, k = 0;
    std::vector<double> r, T;     // the LP's r (L.m), dense T (L.m x n1, row-major)
    std::vector<int> pos_row, pos_col;
    // general stage-2 bounds (twosd_canonical_form): L / r / T above describe the canonical LP
    // (y >= 0, L.m = m2 + nb rows, L.n columns); the caller's sizes, rhs and the back-map of y live
    // here.  has_bounds == false: the template is the caller's own and none of this is read.
    bool has_bounds = false;
    int m2_user = 0, n2_user = 0, nb = 0;
    double c0 = 0.0;              // objective constant q.s of the shift
    std::vector<double> r_user;   // the caller's r (m2_user): scenario values are in its space
    twosd::DevBuf<int> d_bm_src, d_bm_src2;   // n2_user: LP column(s) of each caller column
    twosd::DevBuf<double> d_bm_sign, d_bm_off;
    twosd::DevBuf<double> d_yu;       // y of the last batch in the caller's space (N x n2_user)
    twosd::DevBuf<int> d_colptr, d_rowidx;
    twosd::DevBuf<double> d_val, d_q;
    twosd::DevBuf<int8_t> d_btype;
    twosd::DevBuf<uint64_t> d_fixedmask, d_ubmask;
    // warm-start basis pool (basis_pool.h): host forms, pool-strided device arrays, validity
    twosd::BasisPool bp;
    twosd::DevBuf<double> d_xbase;       // per x: x_B of every pool basis (prepare_x)
    // pool selection data (per x, prepare_x): constant-row infeasibility, active rows, entries
    twosd::DevBuf<float> d_sel_cinf;
    twosd::DevBuf<int> d_sel_ptr, d_sel_code;   // code: (code, float bits) record pairs
    twosd::DevBuf<int> d_sel_end;            // npool: end of each basis's records (begin = d_sel_ptr, static capacity)
    twosd::DevBuf<double> d_xaux;            // per x: b (m), coef (k), box lo (k), box hi (k)
    int64_t sel_cap_total = 0;           // records the static capacity layout holds
    int64_t sel_nnz = 0;
    float sel_cw = 0.0f;                 // pool selection key: sum |infeas| + sel_cw * #infeasible rows (per x)
    std::vector<double> dist_mad;        // mean absolute deviation E|V_e - E V_e| of each random element
    std::vector<double> sel_lo, sel_hi;   // training box of the deltas (empty: no row pruning)
    twosd::DevBuf<int> d_head_out, d_pool_pick;   // optional LP outputs (pool building)
    // two-level pool selection (twosd_pool_build_candidates): level 1 over pool[0, pool_l1),
    // level 2 over the candidate bases of the level-1 pick (d_cand: pool_l1 x pool_ncand)
    int pool_l1 = 0, pool_ncand = 0;
    twosd::DevBuf<int> d_cand;
    // candidate lists of the last refresh, built on the host by the next two-level selection while
    // its level-1 pass runs (select_pool); pool_l1 / pool_ncand already describe them
    std::vector<int> cand_p1, cand_pf;
    int cand_pl1 = 0, cand_pnc = 0;
    bool cand_pending = false;
    twosd::DevBuf<int> d_cpick;       // candidate picks of the training scenarios (grow-only)
    twosd::DevBuf<float> d_sel_key;
    twosd::DevBuf<float> d_sel_pkey;          // chunked selection partials (split x N)
    twosd::DevBuf<int> d_sel_ppick;
    twosd::DevBuf<int> d_order;       // LP visiting order grouped by pool basis
    twosd::DevBuf<char> d_sort_tmp;
    twosd::DevBuf<int2> d_qrec;       // LP launch: (scenario, start basis) per queue position
    bool prep_valid = false;      // the per-x preparation (d_xbase, d_sel_*) matches the pool and prep_x
    twosd::DevBuf<double> d_kcoef;    // k: coef_e(x) = 1 (RHS element) or -x[col] (T element)
    std::vector<double> prep_x;
    // hypersparse kernel data
    int CH = 0;                   // column slots per lane of the hypersparse kernel
    twosd::DevBuf<int> d_wcp, d_wcc;   // W by rows (CSR) for the segmented pricing scatter
    twosd::DevBuf<double> d_wcv;
    twosd::DevBuf<int> d_eidx;
    twosd::DevBuf<double> d_evals;
    size_t earena_slots = 0;      // eta arena (d_eidx, d_evals): LP slots ...
    int earena_cap = 0;           // ... of this many entries each
    twosd::DevBuf<unsigned long long> d_stamps;
    // LP workspace + outputs
    twosd::DevBuf<int> d_queue;
    twosd::DevBuf<unsigned long long> d_lpstats;   // lp_stats_kernel output (5 words)
    twosd::DevBuf<double> d_obj, d_pi, d_y;
    twosd::DevBuf<int> d_status, d_iters;
    twosd::DevBuf<long long> d_ops;
    twosd::DevBuf<int> d_etan;
    int out_cap = 0;              // scenarios the per-scenario LP outputs are sized for (rows of d_pi, d_y, d_vkey, d_bkey)
    twosd::DevBuf<double> d_dvtmp;
    twosd::DevBuf<double> d_objpart;
    // out-of-sample moments (eval_moments_kernel): the blocks' partial records, and a grow-only
    // copy of objectives / statuses (the solve at xa of a paired chunk; moments_of_values' upload)
    twosd::DevBuf<char> d_mompart;
    twosd::DevBuf<double> d_ev_obj;
    twosd::DevBuf<int> d_ev_st;
    // group means and group statuses of a variance-reduced chunk (group_means_kernel; the paired
    // form's second array behind the first)
    twosd::DevBuf<double> d_gm_mean;
    twosd::DevBuf<int> d_gm_st;
    // scenario distributions (on-device sampler)
    bool has_dist = false;
    twosd::DevBuf<int> d_dist_kind, d_dist_off;
    twosd::DevBuf<double> d_dist_val, d_dist_prob, d_dist_p0, d_dist_p1, d_dist_tmpl;
    // joint discrete blocks (twosd_set_distributions_joint; dist_tables.h): per element lead /
    // block / column, per block its record, the running sums and the values
    bool has_blocks = false;
    twosd::DevBuf<int> d_dist_elead, d_dist_eblk, d_dist_ecol;
    twosd::DevBuf<twosd::DistBlock> d_dist_binfo;
    twosd::DevBuf<double> d_dist_bcum, d_dist_bval;
    // LINTR blocks (twosd_set_distributions_lintr; lintr_tables.h, lintr.hip): the M member rows
    // (element, constant, CSR over global latent numbers), the Q latents as an independent layout
    // (their zero template among them), and the grow-only scratch of the latent pass
    bool has_lintr = false;
    int lintr_M = 0, lintr_Q = 0;
    twosd::DevBuf<int> d_lt_elem, d_lt_rptr, d_lt_col;
    twosd::DevBuf<double> d_lt_c, d_lt_h;
    twosd::DevBuf<int> d_lt_kind, d_lt_off, d_lt_word;
    twosd::DevBuf<double> d_lt_val, d_lt_prob, d_lt_p0, d_lt_p1, d_lt_zero;
    twosd::DevBuf<double> d_lt_xi;
    // epigraphs
    std::vector<twosd::EpiDevice> epis;
    // dual vertex set
    twosd::DvsDevice dvs;
    std::unique_ptr<twosd::DvsWs, void (*)(twosd::DvsWs *)> dvs_ws{nullptr, twosd::dvs_free};   // dvs scratch (dvs_kernel.hip)
    // cut workspace (cut_common.h: CutWs)
    std::unique_ptr<twosd::CutWs, void (*)(twosd::CutWs *)> cut_ws{nullptr, twosd::cut_free};
    // the last twosd_build_cut / twosd_cut_partial whose picks still sit in the cut workspace:
    // its epigraph (-1: none, or invalidated since), scenarios (0: the empty-epigraph path), |V|
    int last_cut_epi = -1, last_cut_n = 0, last_cut_nv = 0;
    twosd::ReformState reform;    // stored picks and the buffers of cuts re-formed from picks (reform.hip)
    // dual-vertex key workspace (vkey.hip) and the key output of the LP kernel
    std::unique_ptr<twosd::VkeyWs, void (*)(twosd::VkeyWs *)> vkey_ws{nullptr, twosd::vkey_free};
    twosd::DevBuf<unsigned long long> d_vkey, d_bkey;
    // eta-file output of a pool refresh (list positions x kmax / kmax + 1, shared entry arena)
    twosd::DevBuf<int> d_eo_pb, d_eo_K, d_eo_off, d_eo_etap, d_eo_etaoff;
    twosd::DevBuf<int> d_eo_eidx;
    twosd::DevBuf<unsigned long long> d_eo_used;
    twosd::DevBuf<double> d_eo_evals;
    size_t eo_rows = 0;      // list positions the per-position arrays hold (x eo_kmax / eo_kmax + 1 pivots)
    size_t eo_cap = 0;       // entries of the shared arena (d_eo_eidx and d_eo_evals)
    size_t eo_min_cap = 0;   // arena floor: what a training run whose eta files did not fit asked for
    int eo_kmax = 0;
    double last_refresh_ms[5] = {0, 0, 0, 0, 0};   // train solves, re-solves, compose, upload, total
    twosd::DevBuf<int> d_refresh_sel;                  // refresh: scenarios to re-solve
    twosd::BoxCache sel_box;                           // training range of sel_lo / sel_hi (single-rank refresh)
    // device pool build of a refresh (pool_gpu.hip): intermediate CSC, per-source counts and
    // checks, pool map / offsets, primary head and d0
    twosd::DevBuf<double> d_pg_amax, d_pg_d0p, d_pg_ival;
    twosd::DevBuf<int> d_pg_irow;
    twosd::DevBuf<long long> d_pg_ioff;
    twosd::DevBuf<int> d_pg_cnt, d_pg_tot, d_pg_valid, d_pg_head0;
    twosd::DevBuf<int> d_pg_map, d_pg_off, d_pg_pos;
    // FTRAN results of the first pass kept for the gather (pool_gpu.hip): per source sc_cap entries
    twosd::DevBuf<int> d_pg_scrow, d_pg_scoff;
    twosd::DevBuf<double> d_pg_scval;
    long long pg_sc_cap = 0;                       // entries per source of the last build (0: first build)
    // distributed refresh (twosd_refresh_*, pool_refresh.hip): this rank's training keys, its pack of built
    // sources, and the source table gathered from all ranks
    std::vector<unsigned long long> rt_keys;
    std::vector<int> rt_counts, rt_reps;
    std::vector<double> rt_lo, rt_hi;     // training box of this rank's slice
    twosd::BoxCache rt_box;               // the slice of the last twosd_refresh_train*, the range of rt_lo / rt_hi
    int rt_nown = -1;
    bool rt_trained = false;              // a twosd_refresh_train* ran since the last assemble
    long long rt_nz0 = 0;                 // intermediate entries of the primary (local source 0)
    int rt_nsrc_local = 0;
    twosd::DevBuf<char> d_rt_pack;
    twosd::DevBuf<int> d_gs_heads, d_gs_cnt, d_gs_tot, d_gs_valid, d_gs_irow;
    twosd::DevBuf<long long> d_gs_ioff;
    twosd::DevBuf<double> d_gs_ival;
    twosd::DevBuf<char> d_gs_seg;             // copy-segment list of the gather unpack
    int last_push_reps = 0;       // representatives re-solved by the last solve_push
    double push_rep_frac = 0.0;   // representatives / scenarios of the last keyed solve_push (push mode choice)
    int last_push_full = 0;       // 1: the last solve_push recovered every dual in its main pass
    twosd::DevBuf<double> d_pi_rep;   // the representatives' dual rows gathered for the push (full mode)
    twosd::FrayState fray;        // feasibility ray set and twosd_solve_rays' workspaces (feas.hip)
    twosd::RiskState risk;        // quantile selection and tail cut workspaces (risk.hip)
};

// The context: the template state plus what lives as long as the handle.
struct twosd_ctx : TemplateState {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[twosd::EV_COUNT] = {};   // EventSlot
    int num_cus = 256;
    int kmax_override = 0;
    int train_kcap = 0;           // pivot cap of the refresh training solves (> 0; 0: auto; < 0: none): a caller setting
    twosd::PinnedBuf stage[twosd::STG_COUNT];   // pinned host staging slots of the uploads (StageSlot)
    ~twosd_ctx() {
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
        if (stream) hipStreamDestroy(stream);
    }
};

namespace twosd {
int fail(int code, const char *fmt, ...);
int prepare_x(twosd_ctx *c, const double *x);   // pool_select.hip
// options of run_lp: vertex keys instead of pi (solve_push), or a list of scenarios to
// re-solve from their recorded pool picks with pi at the list position
struct LpRun {
    bool want_pi = false, want_y = false, want_key = false;
    bool want_bkey = false;       // basis keys into c->d_bkey
    bool want_etas = false;       // eta files into c->eo (pool refresh), rows by list position / scenario
    bool want_head = false;       // final heads into c->d_head_out, rows by list position / scenario
    const int *d_list = nullptr;  // list mode: scenarios (indices into d_dv) to solve, no selection
    int nlist = 0;
    int kcap = 0;                 // > 0: pivot cap below kmax, no retry from the primary basis (refresh training)
    double *lp_us_out = nullptr;  // list mode: the launch's LP kernel time (c->last is not written)
    bool want_ray = false;        // list mode only: Farkas rays, leaving rows and ray keys of the infeasible
                                  // scenarios into c->fray.ray / ray_row / ray_key, rows by list position
};
// Launch the LP kernel over N scenarios whose deltas start at d_dv (device); results in
// c->d_obj / d_pi / d_y / d_status / d_iters [0, N) (lp_batch.hip).
int run_lp(twosd_ctx *c, const double *x, const double *d_dv, int N, const LpRun &o = LpRun());
// what one translation unit of the library needs of another (api.hip; pool_select.hip; lp_batch.hip;
// the pool's own are in basis_pool.h); hidden: they were file-local while api.hip held it all, and
// the library's dynamic symbols stay what they were
#pragma GCC visibility push(hidden)
double template_value(const twosd_ctx *c, int e);   // at position e, in the caller's space
void rhs_at(const twosd_ctx *c, const double *x, const double *dv, std::vector<double> &b);   // b = r - T x + deltas
// SampleParams of n scenarios from first_index of stream `seed`, drawn from the context's distributions into out
SampleParams sample_params(const twosd_ctx *c, int n, uint64_t seed, uint64_t first_index, double *out);
// n scenarios from first_index of stream `seed` under the plan (mode, G) into out (n x k deltas), on
// the context's stream: launch_sample_plan, then the LINTR blocks' latent and apply passes (lintr.hip)
int draw_scenarios(twosd_ctx *c, int n, uint64_t seed, uint64_t first_index, double *out, int mode, int G);
int upload_lintr(twosd_ctx *c, const LintrTables &T);   // T.M == 0 drops the LINTR tables
// pick[s] = warm-start basis of scenarios [0, N) at the prepared x, c->d_order = the scenarios grouped by pick
int select_pool(twosd_ctx *c, const double *d_dv, int N, int *d_pick, int npool_override);
// statistics and objective sums of the batch into c->last, outputs to the host (each nullable);
// d_w: the batch's scenario weights (nullable: 1.0).  TWOSD_E_LP when some LP is not optimal.
int copy_lp_outputs(twosd_ctx *c, int N, double *obj, double *pi, double *y, int *status, const double *d_w);
int prepare_elements(twosd_ctx *c);
int reserve_selection(twosd_ctx *c, int P, int records);
void reset_candidates(twosd_ctx *c);
// box [lo, hi] of the deltas of training scenarios [first, first + count) of epigraph epi (E): the
// selection's row pruning.  With a cache, recomputed only when the range differs from the cached one.
int training_box(twosd_ctx *c, const EpiDevice &E, int epi, int first, int count, std::vector<double> &lo,
                 std::vector<double> &hi, BoxCache *cache);
#pragma GCC visibility pop
// f(i) for i in [0, n) on up to 16 host threads (independent work per i); serial when n < serial_below
template <typename F>
void parallel_for(int n, F f, int serial_below = 64) {
    const int nth = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (n < serial_below || nth == 1) {
        for (int i = 0; i < n; ++i) f(i);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < nth; ++t)
        th.emplace_back([&, t]() {
            for (int i = t; i < n; i += nth) f(i);
        });
    for (auto &t : th) t.join();
}
// vkey.hip
int vkey_first_occurrences(twosd_ctx *c, int N, const unsigned long long *d_vkey, const int *d_status, const int **d_list,
                           int *U, const int **d_counts = nullptr);
// dual vertex set (dvs_kernel.hip)
int dvs_init(twosd_ctx *c);
int dvs_push_device(twosd_ctx *c, int count, const double *d_pis, int *d_out_index);
// cut: what other subsystems call (cut_kernel.hip; what the cut's own files share is in cut_common.h)
void cut_invalidate_pk(twosd_ctx *c);
void cut_truncate_pk(twosd_ctx *c, int size);   // V truncated to size: PK rows past it are stale
// The state rule of twosd_picks_keep, twosd_cut_quantile and twosd_cut_tail: a template, an existing
// epigraph, and the last cut built on it with scenarios, its picks and scores still in the cut
// workspace.  who: the caller's name; verb: what it does with the picks ("keep", "read").
int cut_last_usable(twosd_ctx *c, int epi, const char *who, const char *verb);
// for boot_kernel.hip and risk.hip: the picks of the last cut (device, last_cut_n ints), and PK
// (|V| x k4, brought up to date with the vertex set)
const int *cut_last_arg(twosd_ctx *c);
int cut_pk_current(twosd_ctx *c, const double **PK, int *k4);
// for risk.hip: the maximal scores of the last cut (device, last_cut_n doubles, the canonical LP's:
// without c0)
const double *cut_last_val(twosd_ctx *c);
// risk.hip, for twosd_evaluate_cvar (evaluate.hip).  risk_select: the weighted quantile of n
// device-resident values (weights / status nullable; scale: the integer weights' factor), every
// output of twosd_quantile_of_values; TWOSD_E_ARG when no entry counts.  risk_form_y:
// y[i] = var + max(obj[i] - var, 0) / denom in place, each operation rounded on its own.
struct RiskResult { double var, cvar; unsigned long long tail_q, total_q; long long n_bad, n_ok; };
int risk_select(twosd_ctx *c, long long n, const double *d_val, const double *d_w, const int *d_st, double scale, bool has_add,
                double add, double level, const char *who, RiskResult *out);
int risk_form_y(twosd_ctx *c, long long n, double *d_obj, const int *d_st, double var, double denom);
// sampling plans (api.hip): a caller's plan -> (mode, G), NULL meaning i.i.d.; and `what` = value
// must be a whole number of groups.  Both fail with TWOSD_E_ARG and the offending value.
int sampling_plan(const twosd_sampling *plan, const char *who, int *mode, int *G);
int whole_groups(const char *who, const char *what, unsigned long long value, int G);
}  // namespace twosd
