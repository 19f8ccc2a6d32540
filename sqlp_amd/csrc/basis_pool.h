// basis_pool.h -- the warm-start basis pool (basis_pool.hip owns it): the bases in their host
// forms, the pool-strided device arrays the LP kernel, the selection and the refresh read, and
// what says which of them are current.  One member of TemplateState (twosd_ctx::bp).
#pragma once
#include <stdint.h>
#include <vector>
#include "devbuf.h"
#include "pool_pack.h"

struct twosd_ctx;

namespace twosd {
// hidden, types included: the library's dynamic symbols stay what they were
#pragma GCC visibility push(hidden)

// The sixteen pool-strided device arrays, bases[0] first.  Per basis: hb0 (MP), basic0 (64),
// d0 (64 CH), bcp / brptr (MP + 1, absolute into the concatenated bci / bcv and brcol / brval),
// kp (m + 1, absolute into ke / kraw), kslot (R + 1, absolute into kix / kv), bnnz (1).
// The first ten are the pool's own upload (upload_pool); the k* six are the x-independent element
// rows (prepare_elements in pool_select.hip).  A device refresh fills all sixteen (pg_fill_kernel).
struct PoolDev {
    DevBuf<int> hb0;              // 4 head + type, -1 past m
    DevBuf<uint64_t> basic0;      // basic-column masks
    DevBuf<int> bnnz;             // nnz of each B^{-1} (FMA accounting)
    DevBuf<double> d0;            // reduced costs at the basis
    DevBuf<int> bcp, bci;         // B^{-1} by columns (CSC, rows ascending)
    DevBuf<double> bcv;
    DevBuf<int> brptr, brcol;     // B^{-1} by rows (CSR)
    DevBuf<double> brval;
    DevBuf<int> kp, ke;           // element rows, CSR: inputs of the device selection-stream build
    DevBuf<double> kraw;
    DevBuf<int> kslot, kix;       // element rows, sliced ELL: the LP kernel's x_B warm start
    DevBuf<double> kv;
};
// The same sixteen as plain pointers, as they are now (bind again after a reserve): what a kernel
// parameter struct is filled from.  The one list of the pool's arrays besides PoolDev.
struct PoolArrays {
    int *hb0; uint64_t *basic0; int *bnnz; double *d0;
    int *bcp, *bci; double *bcv;
    int *brptr, *brcol; double *brval;
    int *kp, *ke; double *kraw;
    int *kslot, *kix; double *kv;
};

struct BasisPool {
    std::vector<PoolBasis> bases;   // bases[0] = head0 with every host form; see pool_head / pool_host_rows for the rest
    std::vector<int> head0;         // the primary head as installed (twosd_get_basis)
    bool has_basis = false;         // a basis is installed and d matches bases: solves are accepted
    PoolDev d;
    bool k_valid = false;           // d.k* hold the element rows of bases at the current positions
    // the heads of the last device-built pool, fetched on the first host use (P x MP ints, 4 head + type)
    PinnedBuf hb;
    bool hb_valid = false;          // hb holds d.hb0 of the current pool
};

// what the other translation units of the library need of the pool
PoolArrays pool_arrays(const twosd_ctx *c);
// the sixteen arrays sized for P bases with nz B^{-1} entries, kz element entries and ez ELL
// entries in all (grow-only; a grown array does not keep its contents)
int pool_reserve(twosd_ctx *c, int P, size_t nz, size_t kz, size_t ez);
// Lazy host forms.  head of basis p into *head (nullable); a failed read-back drops the pool.
int pool_head(twosd_ctx *c, int p, const std::vector<int> **head);
// every basis of c->bp.bases with head, rptr / rcol / rval and pi0 on the host
int pool_host_rows(twosd_ctx *c);
void pi0_from_rows(const twosd_ctx *c, PoolBasis &B);
// bases -> the ten arrays of the pool's own upload, then pool_installed_from_host
int upload_pool(twosd_ctx *c);
// bases = the primary + the host-form bases fresh[a] with ok[a]; the caller uploads
void pool_replace_host_bases(twosd_ctx *c, std::vector<PoolBasis> &fresh, const std::vector<char> &ok);
// The transitions: the only writers of has_basis, k_valid, hb_valid, hb_row and dev_only.
void pool_installed_from_host(twosd_ctx *c);            // upload_pool wrote bases into the arrays
void pool_installed_from_device(twosd_ctx *c, int P);   // a device refresh filled the arrays with P bases
int pool_dropped(twosd_ctx *c, int code);               // the arrays no longer hold bases; returns code
void pool_elements_ready(twosd_ctx *c);                 // prepare_elements wrote the element rows
void pool_positions_changed(twosd_ctx *c);              // twosd_set_random_positions took new positions
#pragma GCC visibility pop

}  // namespace twosd
