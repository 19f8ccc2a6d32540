// devbuf.h -- the owners of device and pinned host memory (library-internal).  Every allocation
// and free of the library goes through these two types.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include "twosd_hip.h"

namespace twosd {
int fail(int code, const char *fmt, ...);

// TWOSD_POISON=<byte> (test hook): every new device allocation is filled with that byte, so a
// result that depends on memory no kernel wrote changes with it (the fill completes before the
// allocation returns: the context's streams do not order against the null-stream memset).
// TWOSD_POISON_FAMILY selects the allocations by bit: 1 plain allocation, 2 grow-with-keep,
// 4 cut workspace, 8 vkey / dvs workspaces.  Returns the byte, or -1 when off for `family`.
inline int poison_byte(int family) {
    static const int b = getenv("TWOSD_POISON") ? atoi(getenv("TWOSD_POISON")) : -1;
    static const int fam = getenv("TWOSD_POISON_FAMILY") ? atoi(getenv("TWOSD_POISON_FAMILY")) : -1;
    static const bool said = b >= 0 && fprintf(stderr, "TWOSD_POISON: new device allocations filled with 0x%02x (families %d)\n",
                                               b & 0xff, fam) > 0;
    (void)said;
    return (fam & family) ? b : -1;
}

// Move-only owner of a device array: p, and cap = the element count it was last sized for.
// Converts to T* so that reads, pointer arithmetic and kernel arguments take the buffer itself;
// .p is for template deduction and casts.  Family: the poison family of its allocations.
template <typename T, int Family = 1>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); std::swap(p, o.p); std::swap(cap, o.cap); }
        return *this;
    }
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    void release() {
        if (p) hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // exactly count elements (at least one is allocated), contents not kept
    int alloc(size_t count) {
        release();
        int rc = raw(&p, std::max<size_t>(count, 1), Family);
        if (!rc) cap = count;
        return rc;
    }
    // grow-only, exact: sized to n when n elements do not fit; contents not kept
    int fit(size_t n) { return n <= cap ? TWOSD_OK : alloc(n); }
    // grow-only, 25 % slack: no hipFree / hipMalloc when n elements fit; contents not kept
    int reserve(size_t n) {
        n = std::max<size_t>(n, 1);
        return p && cap >= n ? TWOSD_OK : alloc(n + n / 4);
    }
    // exactly count elements, keeping the first `keep` (copied on stream s, which is drained)
    int regrow(size_t count, size_t keep, hipStream_t s) {
        T *np = nullptr;
        if (int rc = raw(&np, count, 2)) return rc;
        if (p && keep) {
            hipError_t e = hipMemcpyAsync(np, p, sizeof(T) * keep, hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) { hipFree(np); return fail(TWOSD_E_DEVICE, "grow copy: %s", hipGetErrorString(e)); }
            hipStreamSynchronize(s);
        }
        release();
        p = np;
        cap = count;
        return TWOSD_OK;
    }
    // at least count elements, keeping the first `keep`; grows to max(count, 2 cap + 1024)
    int grow(size_t count, size_t keep, hipStream_t s) {
        return p && count <= cap ? TWOSD_OK : regrow(std::max<size_t>(count, cap * 2 + 1024), keep, s);
    }
    // n host elements to the front of the buffer
    int copy_from(const T *h, size_t n) {
        if (!n) return TWOSD_OK;
        hipError_t e = hipMemcpy(p, h, sizeof(T) * n, hipMemcpyHostToDevice);
        return e == hipSuccess ? TWOSD_OK : fail(TWOSD_E_DEVICE, "upload of %zu bytes: %s", sizeof(T) * n, hipGetErrorString(e));
    }
    // host -> device into an exact allocation / a grow-only one (reserve)
    int upload(const T *h, size_t n) {
        int rc = alloc(std::max<size_t>(n, 1));
        return rc ? rc : copy_from(h, n);
    }
    int upload(const std::vector<T> &h) { return upload(h.data(), h.size()); }
    int upload_reserve(const T *h, size_t n) {
        int rc = reserve(n);
        return rc ? rc : copy_from(h, n);
    }
    int upload_reserve(const std::vector<T> &h) { return upload_reserve(h.data(), h.size()); }

private:
    static int raw(T **out, size_t count, int family) {
        hipError_t e = hipMalloc((void **)out, sizeof(T) * count);
        if (e != hipSuccess) return fail(TWOSD_E_DEVICE, "hipMalloc(%zu bytes): %s", sizeof(T) * count, hipGetErrorString(e));
        if (poison_byte(family) >= 0) { hipMemset(*out, poison_byte(family), sizeof(T) * count); hipDeviceSynchronize(); }
        return TWOSD_OK;
    }
};

// Move-only owner of a pinned host buffer, grown with 25 % slack and never shrunk.
struct PinnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept {
        if (this != &o) { release(); std::swap(p, o.p); std::swap(bytes, o.bytes); }
        return *this;
    }
    ~PinnedBuf() { release(); }
    void release() {
        if (p) hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
    // at least n elements of T (contents not kept on growth); nullptr when the allocation fails
    template <typename T>
    T *reserve(size_t n) {
        const size_t need = std::max<size_t>(n, 1) * sizeof(T);
        if (need > bytes) {
            release();
            if (hipHostMalloc(&p, need + need / 4) != hipSuccess) { p = nullptr; return nullptr; }
            bytes = need + need / 4;
        }
        return static_cast<T *>(p);
    }
    template <typename T>
    T *as() const { return static_cast<T *>(p); }
};

}  // namespace twosd
