// bn_host.h -- the host toolkit every handle of the library is written with: the device guard, the HIP check that reports through
// the family's own fail function (each bn_*_last_error() keeps its thread_local string), the zero-filling allocation, and the table
// of device buffers a handle fills once in its *_create.  Host code only, internal linkage, no kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <vector>

#include "../../include/benchnav_mppi.h"

// `return fail_fn(BN_ERR_HIP, "<expr>: <hipGetErrorString>")` unless expr succeeds.  A family's alias passes its own #expr as
// `text` (BN_HIP_AS), so that the message holds the expression as written, not as expanded.
#define BN_HIP_AS(fail_fn, expr, text) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail_fn(BN_ERR_HIP, std::string(text) + ": " + hipGetErrorString(e_)); } while (0)
#define BN_HIP_OR(fail_fn, expr) BN_HIP_AS(fail_fn, expr, #expr)

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

// The device buffers of one handle: where each pointer lives in the handle, its size, and the id *_device_buffer hands it out
// under (-1: internal).  The one place a buffer's size is written.
struct DeviceBuffers {
    struct Entry { void **slot; size_t bytes; int id; };
    std::vector<Entry> list;

    template <typename P>
    void add(P **slot, size_t bytes, int id = -1) { list.push_back(Entry{(void **)slot, bytes, id}); }

    template <typename Fail>
    int alloc_all(Fail fail)
    {
        for (const Entry &e : list)
            if (int rc = alloc(e.slot, e.bytes, fail)) return rc;
        return BN_OK;
    }

    void free_all()
    {
        for (const Entry &e : list)
            if (*e.slot) { (void)hipFree(*e.slot); *e.slot = nullptr; }
    }

    bool find(int id, void **ptr, size_t *bytes) const
    {
        for (const Entry &e : list)
            if (e.id == id && id >= 0) { *ptr = *e.slot; *bytes = e.bytes; return true; }
        return false;
    }
};

}  // namespace
}  // namespace bn
