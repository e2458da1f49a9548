// bn_host.h -- the host toolkit every handle of the library is written with, the MPPI planner's included: the device guard, the HIP
// check that reports through the family's own fail function (each bn_*_last_error() keeps its thread_local string), the
// zero-filling allocation, and the table of device buffers, pinned blocks and events a handle fills once in its *_create (and one
// more table per group it builds on first use).  Host code only, internal linkage, no kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/benchnav_mppi.h"

// `return fail_fn(BN_ERR_HIP, "<expr>: <hipGetErrorString>")` unless expr succeeds.  A family's alias passes its own #expr as
// `text` (BN_HIP_AS), so that the message holds the expression as written, not as expanded.
#define BN_HIP_AS(fail_fn, expr, text) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail_fn(BN_ERR_HIP, std::string(text) + ": " + hipGetErrorString(e_)); } while (0)
#define BN_HIP_OR(fail_fn, expr) BN_HIP_AS(fail_fn, expr, #expr)
// An entry point's first line once its arguments are checked: work on `device`, or report why not.
#define BN_ON_DEVICE(fail_fn, device) bn::DeviceGuard guard(device); if (!guard.ok) return fail_fn(BN_ERR_HIP, "hipSetDevice failed")

namespace bn {
namespace {

// Every entry point works on the handle's device and leaves the calling thread's current device as it found it
// (one process may drive several GPUs; torch tracks its own notion of the current device).
struct DeviceGuard {
    int prev = -1;
    bool changed = false, ok = true;
    explicit DeviceGuard(int want)
    {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != want) {
            ok = hipSetDevice(want) == hipSuccess;
            changed = ok;
        }
    }
    ~DeviceGuard() { if (changed) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// device memory filled with zeros; an empty buffer still gets a pointer of its own
template <typename P, typename Fail>
int alloc(P **p, size_t bytes, Fail fail)
{
    BN_HIP_OR(fail, hipMalloc((void **)p, bytes ? bytes : 4));
    BN_HIP_OR(fail, hipMemset(*p, 0, bytes ? bytes : 4));
    return BN_OK;
}

// the library runs on the GPU only: the number of visible devices, or BN_ERR_NO_DEVICE
template <typename Fail>
int count_devices(int *ndev, Fail fail)
{
    if (hipGetDeviceCount(ndev) != hipSuccess || *ndev <= 0) return fail(BN_ERR_NO_DEVICE, "no HIP device visible: no CPU fallback");
    return BN_OK;
}

// *_create's device check: a visible device, and device_id one of them
template <typename Fail>
int open_device(int device_id, Fail fail)
{
    int ndev = 0;
    if (int rc = count_devices(&ndev, fail)) return rc;
    if (device_id < 0 || device_id >= ndev) return fail(BN_ERR_INVALID, "device_id out of range");
    return BN_OK;
}

// What one handle (or one lazily built group of a handle) owns on the device and next to it: device buffers, pinned host blocks
// and events.  Each entry says where the pointer lives in the handle, its size, and the id *_device_buffer hands it out under
// (-1: internal).  The one place a buffer's size is written; *_create fills it, alloc_all / free_all / resize work from it.
struct DeviceBuffers {
    enum Kind { kDevice, kPinned, kEvent, kLater };                   // kLater: a device buffer that its first resize allocates
    struct Entry { void **slot; size_t bytes; int id; Kind kind; unsigned flags; };
    std::vector<Entry> list;
    bool live = false;                       // alloc_all succeeded and free_all has not run: what a lazy group's ensure() asks

    template <typename P>
    void add(P **slot, size_t bytes, int id = -1) { list.push_back(Entry{(void **)slot, bytes, id, kDevice, 0}); }
    template <typename P>
    void add_later(P **slot) { list.push_back(Entry{(void **)slot, 0, -1, kLater, 0}); }
    template <typename P>
    void add_pinned(P **slot, size_t bytes, unsigned flags = hipHostMallocDefault) { list.push_back(Entry{(void **)slot, bytes, -1, kPinned, flags}); }
    void add_event(hipEvent_t *ev, unsigned flags = 0) { list.push_back(Entry{(void **)ev, 0, -1, kEvent, flags}); }

    // Everything or nothing: a failure releases what the earlier entries got.  All are allocated, in the order listed, before any is
    // zero-filled: what the runtime allocates for its first fill then lies behind the handle's buffers, not between them.
    template <typename Fail>
    int alloc_all(Fail fail)
    {
        int rc = BN_OK;
        for (size_t i = 0; i < list.size() && !rc; ++i) rc = alloc_one(list[i], fail);
        for (size_t i = 0; i < list.size() && !rc; ++i) rc = zero_one(list[i], fail);
        if (rc) free_all();
        live = !rc;
        return rc;
    }

    // a group that is built on first use
    template <typename Fail>
    int ensure(Fail fail) { return live ? BN_OK : alloc_all(fail); }

    void free_all()
    {
        for (const Entry &e : list) {
            if (!*e.slot) continue;
            if (e.kind == kDevice || e.kind == kLater) (void)hipFree(*e.slot);
            else if (e.kind == kPinned) (void)hipHostFree(*e.slot);
            else (void)hipEventDestroy((hipEvent_t)*e.slot);
            *e.slot = nullptr;
        }
        live = false;
    }

    // Give a registered device buffer another size (zero-filled; the old contents go).  On failure the slot is null and its size
    // 0: the caller invalidates its own size field before the call and sets it after success, so that the next call resizes again.
    template <typename P, typename Fail>
    int resize(P **slot, size_t bytes, Fail fail)
    {
        for (Entry &e : list) {
            if (e.slot != (void **)slot) continue;
            if (*e.slot) { (void)hipFree(*e.slot); *e.slot = nullptr; }
            e.bytes = 0;
            if (int rc = alloc(e.slot, bytes, fail)) return rc;
            e.bytes = bytes;
            return BN_OK;
        }
        return fail(BN_ERR_INVALID, "resize of a buffer that is not in the table");
    }

    bool find(int id, void **ptr, size_t *bytes) const
    {
        for (const Entry &e : list)
            if (e.id == id && id >= 0) { *ptr = *e.slot; *bytes = e.bytes; return true; }
        return false;
    }

private:
    template <typename Fail>
    static int alloc_one(const Entry &e, Fail fail)
    {
        if (e.kind == kDevice) BN_HIP_OR(fail, hipMalloc(e.slot, e.bytes ? e.bytes : 4));
        if (e.kind == kPinned) BN_HIP_OR(fail, hipHostMalloc(e.slot, e.bytes ? e.bytes : 4, e.flags));
        if (e.kind == kEvent) BN_HIP_OR(fail, hipEventCreateWithFlags((hipEvent_t *)e.slot, e.flags));
        return BN_OK;
    }

    template <typename Fail>
    static int zero_one(const Entry &e, Fail fail)
    {
        if (e.kind == kDevice) BN_HIP_OR(fail, hipMemset(*e.slot, 0, e.bytes ? e.bytes : 4));
        if (e.kind == kPinned) std::memset(*e.slot, 0, e.bytes ? e.bytes : 4);
        return BN_OK;
    }
};

}  // namespace
}  // namespace bn
