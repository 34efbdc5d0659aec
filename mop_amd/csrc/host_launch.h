// Host-side plumbing every entry point of libmopk shares: the launch status, pointer tests, and the launcher of kernels whose
// dynamic LDS may exceed the 64 KB default.  Plain inline C++, no device code ("Host launch header").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/mopk.h"

namespace mopk {

// MOPK_OK, or MOPK_ERR_LAUNCH when a launch since the last call failed (this clears HIP's error state)
inline int launch_status() { return hipGetLastError() == hipSuccess ? MOPK_OK : MOPK_ERR_LAUNCH; }

// true when some pointer of the list has a bit of `mask` set (mask = alignment - 1).  A null pointer passes: whether a field may be
// absent is any_null's business, asked where the entry point's check order says so.
template <typename... P> inline bool misaligned(uintptr_t mask, const P *...p) { return (... || (((uintptr_t)p & mask) != 0)); }
template <typename... P> inline bool any_null(const P *...p) { return (... || (p == nullptr)); }
// views (MopkView4 / MopkView5) read or written with 16-byte vectors: each pointer on a 16-byte boundary, each batch / head / row
// stride a multiple of `al` elements
template <typename... View> inline bool views_aligned16(int64_t al, const View &...v) {
    return (... && (!misaligned(15, v.ptr) && v.sb % al == 0 && v.sh % al == 0 && v.sn % al == 0));
}

// Launch KFN with `lds` bytes of dynamic LDS, raising its hipFuncAttributeMaxDynamicSharedMemorySize first when `lds` exceeds
// what this (kernel instantiation, device) pair was last given.  The raised limit is sticky and may NOT be set during stream
// capture: callers warm every shape up before they capture.  One table per instantiation (the template argument), one entry per
// device; a device past the table sets the attribute on every call.  Two host threads that race here both set a sufficient
// value (the entries are atomics, so that is no data race).  Whether the runtime itself keeps the attribute per device is not
// relied on.
constexpr int BIG_LDS_DEVS = 64;
template <auto KFN, typename... Args>
inline int launch_big_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args) {
    static std::atomic<size_t> lds_set[BIG_LDS_DEVS] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return MOPK_ERR_LAUNCH;
    std::atomic<size_t> *const seen = dev >= 0 && dev < BIG_LDS_DEVS ? &lds_set[dev] : nullptr;
    if (!seen || seen->load(std::memory_order_relaxed) < lds) {
        if (hipFuncSetAttribute((const void *)KFN, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return MOPK_ERR_LAUNCH;
        if (seen) seen->store(lds, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(KFN, grid, block, lds, st, args...);
    return launch_status();
}

}  // namespace mopk
