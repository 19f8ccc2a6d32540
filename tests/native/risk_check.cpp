// risk_check.cpp -- the quantile selection's host arithmetic (sqlp_amd/csrc/risk_keys.h) on the
// CPU: prints, for `key` lines given on the command line as hex bit patterns, the key and the
// round trip, and for `thr` lines (level as a hex bit pattern, Q in decimal) the exact threshold
// ceil(level Q).  Built with ASan + UBSan (`make sanitize_risk`); tests/test_risk_host.py compares
// every line with the Python restatement (tests/risk_ref.py).
//   risk_check key <hex bits> ...      ->  key <bits> <key> <bits of unkey(key)>
//   risk_check thr <hex level> <Q> ... ->  thr <hex level> <Q> <t>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "risk_keys.h"

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    if (!strcmp(argv[1], "key")) {
        for (int i = 2; i < argc; ++i) {
            const uint64_t bits = strtoull(argv[i], nullptr, 16);
            double v;
            memcpy(&v, &bits, sizeof v);
            const uint64_t k = twosd::risk_key(v);
            const double back = twosd::risk_unkey(k);
            uint64_t bb;
            memcpy(&bb, &back, sizeof bb);
            printf("key %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits, k, bb);
        }
        return 0;
    }
    if (!strcmp(argv[1], "thr")) {
        for (int i = 2; i + 1 < argc; i += 2) {
            const uint64_t bits = strtoull(argv[i], nullptr, 16);
            double level;
            memcpy(&level, &bits, sizeof level);
            const uint64_t Q = strtoull(argv[i + 1], nullptr, 10);
            printf("thr %016" PRIx64 " %" PRIu64 " %" PRIu64 "\n", bits, Q, twosd::risk_threshold(level, Q));
        }
        return 0;
    }
    return 2;
}
