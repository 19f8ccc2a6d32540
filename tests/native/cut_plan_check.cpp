// The cut's launch plan on the CPU (ASan + UBSan): includes cut_plan.h alone and prints the plan of
// a table of shapes, one line each, for tests/test_cut_plan_host.py.
//   plan N nv k cus bpc [knob] : <fields>     or     plan ... : refused envelope | refused log
#include <cstdio>
#include "cut_plan.h"

using namespace twosd;

// the argmax kernels' k-block instantiations (cut_common.h: kCutKBs)
static const int kKBs[] = {1, 2, 4, 6, 8, 12, 16, 22, 24, 30, 32};
static const int kNKB = sizeof(kKBs) / sizeof(kKBs[0]);

static void show(const CutShape &sh, const CutKnobs &kn, const char *note) {
    CutPlan p;
    printf("plan %d %d %d %d %d %s :", sh.N, sh.nv, sh.k, sh.num_cus, sh.bpc, note);
    switch (cut_plan(sh, kn, kKBs, kNKB, p)) {
    case CUT_PLAN_K_ENVELOPE: printf(" refused envelope\n"); return;
    case CUT_PLAN_LOG_SLOTS: printf(" refused log cand_need=%zu tcand_need=%zu\n", p.cand_need, p.tcand_need); return;
    case CUT_PLAN_OK: break;
    }
    printf(" full=%d S=%d nunits=%d nblocks=%d fx_gs=%d fix_blocks=%d ntail=%d merge_blocks=%d resc_blocks=%d slots=%zu"
           " slot_fix=%d slot_merge=%d slot_rescan=%d cand_need=%zu tcand_need=%zu"
           " ntiles=%d nchunks=%d hist_lds=%d k4=%d KB=%d KB32=%d KS8=%d want32=%d wanti8=%d vcap32=%d rows=%d rows32=%d\n",
           p.full, p.S, p.nunits, p.nblocks, p.fx_gs, p.fix_blocks, p.ntail, p.merge_blocks, p.resc_blocks, p.slots, p.slot_fix,
           p.slot_merge, p.slot_rescan, p.cand_need, p.tcand_need, p.ntiles, p.nchunks, p.hist_lds, p.k4, p.KB, p.KB32, p.KS8,
           (int)p.want32, (int)p.wanti8, p.vcap32, p.rows, p.rows32);
}

int main() {
    const CutKnobs def;   // nothing set in the environment
    const CutShape table[] = {
        {1, 1, 0, 256, 3},          {300, 40, 3, 256, 3},       {1000, 256, 5, 256, 3},    {1000, 257, 5, 256, 3},
        {100000, 1000, 86, 256, 3}, {100000, 1000, 86, 256, 2}, {1000000, 5000, 117, 256, 3}, {98304, 2048, 8, 256, 3},
        {98305, 2048, 8, 256, 3},   {125000, 260, 8, 256, 3},
        {67108864, 32, 1, 256, 3},   // 2^32 candidate-log slots: one past the 32-bit offsets
        {1000, 64, 127, 256, 3},    {1000, 64, 128, 256, 3},    // the envelope's last k and the first past it
    };
    for (const CutShape &sh : table) show(sh, def, "default");
    CutKnobs no_tail = def;
    no_tail.tail_split = false;
    show(CutShape{1000000, 5000, 117, 256, 3}, no_tail, "tail=0");
    CutKnobs small_log = def;
    small_log.log_max = 4096;
    show(CutShape{300, 40, 3, 256, 3}, small_log, "log_max=4096");
    CutKnobs no_i8 = def, no_f32 = def;
    no_i8.i8 = false;
    no_f32.f32 = false;
    show(CutShape{300, 40, 3, 256, 3}, no_i8, "i8=0");
    show(CutShape{300, 40, 3, 256, 3}, no_f32, "f32=0");
    for (int k = 0; k <= 127; ++k) {   // KS8 and the k-block choice over the whole envelope
        CutPlan p;
        if (!cut_plan_passes(k, def, kKBs, kNKB, p)) return 1;
        printf("passes k=%d k4=%d KB=%d KB32=%d KS8=%d\n", k, p.k4, p.KB, p.KB32, p.KS8);
    }
    return 0;
}
