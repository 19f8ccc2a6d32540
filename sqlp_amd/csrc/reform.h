// reform.h -- what the bootstrap re-formation (boot_kernel.hip) and the tail cut (risk.hip) share
// on the device (reform.hip).
#pragma once
#include "twosd_ctx.h"
#include "reform_layout.h"

namespace twosd {

// q = rn(w scale), scale = kReformFix / total weight; NaN and w <= 0 weigh nothing
__device__ __forceinline__ unsigned long long reform_q(double w, double scale) {
    return w > 0.0 ? (unsigned long long)__double2ull_rn(w * scale) : 0ull;
}

#pragma GCC visibility push(hidden)
// The handle table (boot_kernel.hip; risk.hip's tail handles share it): a free slot of it, made live by
// the caller; and a usable handle, or the error code with its message (what: the caller's name)
PickSet *pick_slot(twosd_ctx *c, int *id);
int usable_pick(twosd_ctx *c, int handle, const char *what, PickSet **out);
// Before the first reform_finalize_block of a call: the template's device copies (once per
// template) and room in ReformState for B x H output rows and the g partials over nvs vertices.
int reform_prepare(twosd_ctx *c, int B, int H, int nvs);
// out[i] = sum over the chunks of slots[chunk][i], i < width: eight segments of consecutive chunks side by side, then the
// segments in order (the bootstrap), or plain chunk order (the tail cut); they differ above 8 chunks: neither caller may switch
void reform_sum_shards(twosd_ctx *c, bool eight_segments, int nchunks, int width, const double *slots, double *out);
// The finalize stage of handle j of H with B rows: g from the per-vertex integer weights (hist: B
// rows of stride nvs over nv vertices; row 0 weighs every picked vertex), then per row b
//   alpha = (g.r + sum_{e rhs} S[b][e]) / Wq[b] (+ c0),  beta = (-T'g - sum_{e in T} S[b][e] e_col(e)) / Wq[b],
//   weight_mark = Wq[b] wunit;   Wq[b] = 0: the zero cut with weight_mark 0
// into ReformState::d_alpha / d_beta / d_wm at row b * H + j.  Launches only: the caller copies.
int reform_finalize_block(twosd_ctx *c, int B, int H, int j, int nv, int nvs, const unsigned long long *hist, const double *S,
                          const unsigned long long *Wq, double wunit);
#pragma GCC visibility pop

}  // namespace twosd
