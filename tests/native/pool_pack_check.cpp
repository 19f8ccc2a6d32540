// The pool's packing step on the CPU (ASan + UBSan): includes pool_pack.h alone, packs two small
// bases into exactly-sized heap arrays and prints every output array, one line each, for
// tests/test_pool_pack_host.py (which holds the expected values).
//   <case> <array> : v v v ...
#include <cstdio>
#include <memory>
#include <type_traits>
#include "pool_pack.h"

using namespace twosd;

template <typename T>
static void show(const char *name, const char *arr, const T *v, size_t n) {
    printf("%s %s :", name, arr);
    for (size_t i = 0; i < n; ++i) {
        if constexpr (std::is_floating_point<T>::value) printf(" %.17g", (double)v[i]);
        else printf(" %lld", (long long)v[i]);
    }
    printf("\n");
}

// every output exactly as large as the layout says: a write past an end is an ASan report
static void run(const char *name, const HostLP &L, const std::vector<int8_t> &bt, const PoolBasis &B, int MP, int CH, int base) {
    const size_t nz = B.rcol.size();
    std::unique_ptr<int[]> hb(new int[MP]), rp(new int[MP + 1]), cp(new int[MP + 1]), rc(new int[nz]), ci(new int[nz]);
    std::unique_ptr<uint64_t[]> basic(new uint64_t[64]);
    std::unique_ptr<double[]> rv(new double[nz]), cv(new double[nz]), d0(new double[(size_t)64 * CH]);
    for (int i = 0; i < 64; ++i) basic[i] = ~0ull;   // the packing step owns its words: no reliance on a zeroed buffer
    pool_pack_basis(L, bt.data(), B, MP, CH, base, PoolPackOut{hb.get(), basic.get(), rp.get(), rc.get(), rv.get(), cp.get(), ci.get(), cv.get(), d0.get()});
    show(name, "hb", hb.get(), MP);
    show(name, "basic", basic.get(), 64);
    show(name, "rp", rp.get(), MP + 1);
    show(name, "rc", rc.get(), nz);
    show(name, "rv", rv.get(), nz);
    show(name, "cp", cp.get(), MP + 1);
    show(name, "ci", ci.get(), nz);
    show(name, "cv", cv.get(), nz);
    show(name, "d0", d0.get(), (size_t)64 * CH);
}

static std::vector<int8_t> bound_types(const HostLP &L) {   // BT_Y = 0, BT_G = 1, BT_L = 2, BT_E = 3
    std::vector<int8_t> bt(L.n + L.m, 0);
    for (int i = 0; i < L.m; ++i) bt[L.n + i] = L.sense[i] == 'G' ? 1 : (L.sense[i] == 'L' ? 2 : 3);
    return bt;
}

int main() {
    {   // m = 3, n = 4: rows E, G, L; W = [2 0 2 0; 0 1 0 1; 1 1 0 0]; basis {y0, y3, slack of row 2}
        HostLP L;
        L.m = 3; L.n = 4;
        L.colptr = {0, 2, 4, 5, 6};
        L.rowidx = {0, 2, 1, 2, 0, 1};
        L.val = {2, 1, 1, 1, 2, 1};
        L.q = {1, 5, 3, 4};
        L.sense = {'E', 'G', 'L'};
        PoolBasis B;
        B.head = {0, 3, 6};
        B.rptr = {0, 1, 2, 4};                 // B^{-1} = [0.5 0 0; 0 1 0; -0.5 0 1]
        B.rcol = {0, 1, 0, 2};
        B.rval = {0.5, 1, -0.5, 1};
        B.pi0 = {0.5, 4, 0};                   // c_B = (1, 4, 0)
        run("small", L, bound_types(L), B, 64, 1, 5);
    }
    {   // m = 65, n = 2 (MP = 128, two lane slots): basis {y0 in position 3, every slack but row 3's};
        // B^{-1} = I with one more entry, -4 at (64, 3)
        HostLP L;
        L.m = 65; L.n = 2;
        L.colptr = {0, 2, 4};
        L.rowidx = {3, 64, 3, 10};
        L.val = {1, 4, 2, 1};
        L.q = {3, 7};
        L.sense.assign(65, 'L');
        L.sense[0] = 'E';
        L.sense[64] = 'G';
        PoolBasis B;
        B.rptr.push_back(0);
        for (int i = 0; i < 65; ++i) {
            B.head.push_back(i == 3 ? 0 : 2 + i);
            if (i == 64) { B.rcol.push_back(3); B.rval.push_back(-4.0); }
            B.rcol.push_back(i);
            B.rval.push_back(1.0);
            B.rptr.push_back((int)B.rcol.size());
        }
        B.pi0.assign(65, 0.0);
        B.pi0[3] = 3.0;                        // c_B = 3 e_3
        run("slots", L, bound_types(L), B, 128, 2, 7);
    }
    return 0;
}
