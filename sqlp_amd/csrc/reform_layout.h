// reform_layout.h -- the sizes of a cut re-formed from stored picks (reform.hip, boot_kernel.hip,
// risk.hip) as plain arithmetic on counts.  No HIP: tests/native/reform_layout_check.cpp compiles it
// with the host compiler under ASan + UBSan.  The bits of every re-formed cut depend on these.
#pragma once
#include <stddef.h>
#include <algorithm>

namespace twosd {

// q_s = rn(w_s kReformFix / total_weight).  2^58: a Poisson(1) count is at most 12 and
// 12 * 2^58 < 2^62, so every sum of count x q_s over an epigraph is exact in uint64.
constexpr double kReformFix = 288230376151711744.0;

// The S sums of n scenarios are formed per shard of tpb 64-scenario tiles, nchunks shards in all: at
// most four tiles per shard until that makes more than 512 shards, then 512 or fewer equal ones.  A
// function of n alone.  Precondition: n >= 1 (a pick set and a last cut with picks hold a scenario).
// A tail handle's S sums are sharded over its compact list: n = nt list entries, in tiles of 64
// entries; an empty list (nt = 0) has no shards and is never passed here.
constexpr int kReformMaxChunks = 512;
struct ReformShards { int tpb, nchunks; };
inline ReformShards reform_shards(int n) {
    const int ntiles = (n + 63) / 64;
    const int want = std::min(kReformMaxChunks, (ntiles + 3) / 4);
    const int tpb = (ntiles + want - 1) / want;
    return {tpb, (ntiles + tpb - 1) / tpb};
}

// g is formed per chunk of consecutive vertices, the nbc chunks then added in chunk order: 32
// vertices or more per chunk, at most 256 chunks, one for an empty set
struct ReformVertexChunks { int chunk, nbc; };
inline ReformVertexChunks reform_vertex_chunks(int nv) {
    const int chunk = std::max(32, (nv + 255) / 256);
    return {chunk, std::max(1, (nv + chunk - 1) / chunk)};
}

// the partial buffers of H handles with B = M + 1 rows (row 0: the identity replicate) --
//   u64: [B totals][H x B W_jb][H x B x nvs per-vertex weights]     f64: H x B x k S sums (at least 1)
// a tail handle's words are a pick handle's: its W word the tail's weight, its histogram rows, its S sums
struct BootLayout {
    int H, B, nvs, k;
    size_t o_wj, o_hist, n_u64, n_f64;
};
inline BootLayout boot_offsets(int H, int M, int nvs, int k) {
    const size_t B = (size_t)M + 1, o_hist = B + H * B;
    return {H, M + 1, nvs, k, B, o_hist, o_hist + H * B * nvs, std::max<size_t>(H * B * k, 1)};
}

}  // namespace twosd
