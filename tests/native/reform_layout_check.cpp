// reform_layout_check.cpp -- the layouts of a cut re-formed from stored picks
// (sqlp_amd/csrc/reform_layout.h) on the CPU: the shard layout of the S sums, the vertex chunks of
// the g partials and the offsets of the partial buffers, for the sizes given on the command line.
// Built with ASan + UBSan (`make sanitize_reform`); tests/test_reform_layout_host.py compares every
// number with a Python restatement of the formulas.
//   reform_layout_check shard <n> ...             ->  shard <n> <tpb> <nchunks>
//   reform_layout_check vchunk <nv> ...           ->  vchunk <nv> <chunk> <nbc>
//   reform_layout_check off <H> <M> <nvs> <k> ... ->  off <H> <M> <nvs> <k> <B> <o_wj> <o_hist> <n_u64> <n_f64>
//   reform_layout_check fix                       ->  fix <hex bits of the fixed-point scale> <max chunks>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "reform_layout.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "fix")) {
        uint64_t bits;
        const double f = twosd::kReformFix;
        memcpy(&bits, &f, sizeof bits);
        printf("fix %016" PRIx64 " %d\n", bits, twosd::kReformMaxChunks);
        return 0;
    }
    if (!strcmp(argv[1], "shard")) {
        for (int i = 2; i < argc; ++i) {
            const int n = atoi(argv[i]);
            if (n < 1) return 2;   // the header's precondition
            const twosd::ReformShards s = twosd::reform_shards(n);
            printf("shard %d %d %d\n", n, s.tpb, s.nchunks);
        }
        return 0;
    }
    if (!strcmp(argv[1], "vchunk")) {
        for (int i = 2; i < argc; ++i) {
            const int nv = atoi(argv[i]);
            const twosd::ReformVertexChunks v = twosd::reform_vertex_chunks(nv);
            printf("vchunk %d %d %d\n", nv, v.chunk, v.nbc);
        }
        return 0;
    }
    if (!strcmp(argv[1], "off")) {
        for (int i = 2; i + 3 < argc; i += 4) {
            const int H = atoi(argv[i]), M = atoi(argv[i + 1]), nvs = atoi(argv[i + 2]), k = atoi(argv[i + 3]);
            const twosd::BootLayout L = twosd::boot_offsets(H, M, nvs, k);
            printf("off %d %d %d %d %d %zu %zu %zu %zu\n", H, M, nvs, k, L.B, L.o_wj, L.o_hist, L.n_u64, L.n_f64);
        }
        return 0;
    }
    return 2;
}
