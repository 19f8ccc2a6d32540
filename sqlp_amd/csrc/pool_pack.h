// pool_pack.h -- one warm-start basis in its host forms, and the pure packing step that turns it
// into the pool-strided words the LP kernel reads.  Standard library only (no HIP): basis_pool.hip
// calls it per basis, tests/native/pool_pack_check.cpp runs it on the CPU under ASan + UBSan.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace twosd {

// the stage-2 LP on the host (host_basis.cpp): min q'y, W y (sense) b, y >= 0
struct HostLP {
    int m = 0, n = 0;
    std::vector<int> colptr, rowidx;   // W CSC, 0-based
    std::vector<double> val, q;
    std::vector<char> sense;           // 'G','L','E'
};

// one warm-start basis of the pool (bases[0] is the primary basis head0)
struct PoolBasis {
    std::vector<int> head;        // m basic columns (0-based over [y; slacks])
    std::vector<double> Binv;     // m x m row-major
    std::vector<double> pi0;      // c_B' B^{-1}
    std::vector<int> rptr, rcol;  // B^{-1} rows, CSR (|v| > 1e-14 max|B^{-1}|)
    std::vector<double> rval;
    // Private to basis_pool.hip (the lazy host forms of a device-built basis); every other reader
    // gets head through pool_head and rptr / rcol / rval / pi0 through pool_host_rows.
    bool dev_only = false;        // built on the device (refresh): rptr / rcol / rval / pi0 are
                                  // fetched from the pool arrays when the host needs them
    int hb_row = -1;              // >= 0: head not materialised yet; row of BasisPool::hb (4 head + type)
};

// where pool_pack_basis writes one basis: its own slice of every pool-strided array
struct PoolPackOut {
    int *hb;                      // MP: 4 head + type, -1 past m
    uint64_t *basic;              // 64: bit (j >> 6) of word (j & 63) set for every basic column j
    int *rp, *rc; double *rv;     // B^{-1} CSR: MP + 1 pointers; the basis's entries
    int *cp, *ci; double *cv;     // B^{-1} CSC (rows ascending within a column), likewise
    double *d0;                   // 64 CH reduced costs q_j - pi0'a_j, 0 for basic / padding columns (CH <= 0: unread)
};

// The hypersparse-kernel form of basis B of LP L (bt: bound type of each of the n + m columns).
// rp / cp are absolute into the pool's concatenated entry arrays, where this basis's entries
// start at `base`; both are padded to MP + 1 with their last value.  (Hidden: the library's
// dynamic symbols stay what they were.)
__attribute__((visibility("hidden"))) inline void pool_pack_basis(const HostLP &L, const int8_t *bt, const PoolBasis &B, int MP, int CH, int base, const PoolPackOut &o) {
    const int m = L.m, n = L.n;
    std::vector<char> isb(n + m, 0);
    std::fill(o.basic, o.basic + 64, (uint64_t)0);
    for (int i = 0; i < m; ++i) {
        o.hb[i] = B.head[i] * 4 + bt[B.head[i]];
        o.basic[B.head[i] & 63] |= 1ull << (B.head[i] >> 6);
        isb[B.head[i]] = 1;
    }
    for (int i = m; i < MP; ++i) o.hb[i] = -1;
    for (int i = 0; i <= MP; ++i) o.rp[i] = base + B.rptr[std::min(i, m)];
    std::copy(B.rcol.begin(), B.rcol.end(), o.rc);
    std::copy(B.rval.begin(), B.rval.end(), o.rv);
    // columns: counting sort of the row CSR (rows ascending within a column)
    std::vector<int> pos(m + 1, 0);
    for (int cc : B.rcol) ++pos[cc + 1];
    for (int cc = 0; cc < m; ++cc) pos[cc + 1] += pos[cc];
    for (int cc = 0; cc <= MP; ++cc) o.cp[cc] = base + pos[std::min(cc, m)];
    for (int i = 0; i < m; ++i)
        for (int q = B.rptr[i]; q < B.rptr[i + 1]; ++q) {
            const int at = pos[B.rcol[q]]++;
            o.ci[at] = i;
            o.cv[at] = B.rval[q];
        }
    if (CH <= 0) return;
    for (int j = 0; j < 64 * CH; ++j) {
        if (j >= n + m || isb[j]) { o.d0[j] = 0.0; continue; }
        double sum = 0.0;
        if (j >= n) sum = B.pi0[j - n];
        else
            for (int q = L.colptr[j]; q < L.colptr[j + 1]; ++q) sum += B.pi0[L.rowidx[q]] * L.val[q];
        o.d0[j] = (j < n ? L.q[j] : 0.0) - sum;
    }
}

}  // namespace twosd
