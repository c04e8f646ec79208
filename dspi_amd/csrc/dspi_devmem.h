// dspi_devmem.h — who owns a context's device memory: grow-only buffers that register with one DevMem (walking it is the single release
// path), the pinned host areas, and the table of the persistent per-stream arrays with their byte arithmetic.  Plain C++ (no HIP): the
// allocator is a template parameter, so dspi_capi.cpp passes its HIP policy and tests/devmem_driver.cpp a fake that records every call.
//
// An allocator A answers true = done:  dev_alloc(void **p, size_t bytes)  dev_free(void *p)  dev_copy(void *dst, const void *src, size_t bytes)
//                                      host_alloc(void **p, size_t bytes) host_free(void *p) host_device_ptr(void **dp, void *hp)
// Frees must wait for the device (hipFree, hipHostFree): a buffer is grown while earlier asynchronous work may still be using the old one.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dspi_image.h"

namespace dspi {

struct DevMem;
// one owned allocation; it joins its DevMem once, at construction, behind everything constructed before it, and never moves
struct MemNode {
    void *p = nullptr;
    size_t cap = 0;            // bytes
    void *dev = nullptr;       // pinned areas: the device's address of p, where one was asked for
    const bool pinned;
    MemNode *next = nullptr;
    MemNode(DevMem &m, bool pinned_area);
    MemNode(const MemNode &) = delete;
    MemNode &operator=(const MemNode &) = delete;
};
// the registry.  It has no destructor on purpose: its owner says when the memory goes (devmem_release), with the right device current.
struct DevMem { MemNode *first = nullptr, *last = nullptr; };
inline MemNode::MemNode(DevMem &m, bool pinned_area) : pinned(pinned_area) { (m.last ? m.last->next : m.first) = this; m.last = this; }

// a device buffer, read like the T * it holds (a member load)
template <class T> struct DevBuf : MemNode {
    explicit DevBuf(DevMem &m) : MemNode(m, false) {}
    T *get() const { return static_cast<T *>(p); }
    operator T *() const { return get(); }
};
// a pinned host area, read like the host's T *; device(): the same bytes as the kernels address them
template <class T> struct PinnedBuf : MemNode {
    explicit PinnedBuf(DevMem &m) : MemNode(m, true) {}
    T *get() const { return static_cast<T *>(p); }
    operator T *() const { return get(); }
    T *device() const { return static_cast<T *>(dev); }
};

enum class Mem { Ok, FreeFailed, AllocFailed, CopyFailed, NoDevicePtr };

// at least `bytes`: a request that fits does nothing; else the buffer is freed, then exactly `bytes` are allocated (contents are not kept).
// A failed free leaves the buffer as it was, a refused allocation {nullptr, 0}.
template <class A> Mem devmem_grow(A &a, MemNode &b, size_t bytes) {
    if (bytes <= b.cap) return Mem::Ok;
    if (b.p && !a.dev_free(b.p)) return Mem::FreeFailed;
    b.p = nullptr; b.cap = 0;
    if (!a.dev_alloc(&b.p, bytes)) { b.p = nullptr; return Mem::AllocFailed; }
    b.cap = bytes;
    return Mem::Ok;
}
// ... keeping the contents: allocate, copy the old bytes device to device, free the old buffer.  Refused, or the copy failed: the old buffer stays.
template <class A> Mem devmem_grow_keep(A &a, MemNode &b, size_t bytes) {
    if (bytes <= b.cap) return Mem::Ok;
    void *fresh = nullptr, *const old = b.p;
    if (!a.dev_alloc(&fresh, bytes)) return Mem::AllocFailed;
    if (old && !a.dev_copy(fresh, old, b.cap)) { a.dev_free(fresh); return Mem::CopyFailed; }
    b.p = fresh; b.cap = bytes;
    return old && !a.dev_free(old) ? Mem::FreeFailed : Mem::Ok;
}
// a pinned area of at least `bytes`: one that is too small is replaced by one of `grow` >= bytes; device_ptr: b.dev is asked for too
template <class A> Mem devmem_grow_pinned(A &a, MemNode &b, size_t bytes, size_t grow, bool device_ptr) {
    if (bytes <= b.cap) return Mem::Ok;
    if (b.p && !a.host_free(b.p)) return Mem::FreeFailed;
    b.p = b.dev = nullptr; b.cap = 0;
    if (!a.host_alloc(&b.p, grow)) { b.p = nullptr; return Mem::AllocFailed; }
    if (device_ptr && !a.host_device_ptr(&b.dev, b.p)) { a.host_free(b.p); b.p = b.dev = nullptr; return Mem::NoDevicePtr; }
    b.cap = grow;
    return Mem::Ok;
}
// every live buffer once, in registration order; what is empty (never grown, refused, released before) is passed over
template <class A> void devmem_release(A &a, DevMem &m) {
    for (MemNode *n = m.first; n; n = n->next) {
        if (n->p) (void)(n->pinned ? a.host_free(n->p) : a.dev_free(n->p));
        n->p = n->dev = nullptr; n->cap = 0;
    }
}

// ---- the persistent per-stream arrays: stacks of rows, row-outermost (dspi_resize.h), allocated for the context's row capacity ----
enum PersistArray : int { kArrState = 0, kArrLines, kArrRing, kArrPdm, kArrPdmBase, kNumPersist };
struct PersistInfo {
    const char *name;
    size_t (*row_bytes)(const StateMap &);
    bool at_create;            // else on first use (the modulator's first run, the fade mode's first enable), and absent until then
};
extern const PersistInfo kPersist[kNumPersist];
// the bytes of `rows` rows of array k; false where they do not fit a size_t
bool persist_bytes(int k, const StateMap &sm, uint32_t rows, size_t *bytes);
// ... do for every array of the table
bool persist_rows_fit(const StateMap &sm, uint32_t rows);

// New arrays of `rows` rows for those of arr[] that exist, all or nothing: EVERY one is allocated before anything else happens (a refusal
// frees what was made and leaves arr[] and cap_rows alone); copy(fresh) brings the rows in use over and waits for them, once; then the old
// arrays are freed and replaced, and cap_rows changes last.
template <class A, class Copy> Mem persist_reallocate(A &a, MemNode *const arr[kNumPersist], const StateMap &sm, uint32_t rows, uint32_t &cap_rows, Copy copy) {
    void *fresh[kNumPersist] = {};
    size_t bytes[kNumPersist] = {};
    auto drop = [&]() { for (void *f : fresh) if (f) a.dev_free(f); };
    for (int k = 0; k < kNumPersist; k++)
        if (arr[k]->p && (!persist_bytes(k, sm, rows, &bytes[k]) || !a.dev_alloc(&fresh[k], bytes[k]))) { fresh[k] = nullptr; drop(); return Mem::AllocFailed; }
    if (!copy(fresh)) { drop(); return Mem::CopyFailed; }
    for (int k = 0; k < kNumPersist; k++)
        if (fresh[k]) { a.dev_free(arr[k]->p); arr[k]->p = fresh[k]; arr[k]->cap = bytes[k]; }
    cap_rows = rows;
    return Mem::Ok;
}

}  // namespace dspi
