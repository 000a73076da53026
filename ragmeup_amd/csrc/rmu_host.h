// rmu_host.h -- the host plumbing every unit of librmu.so is built from (include after rmu_common.h): the error path, the "runtime is
// winding down" flag, the grow-only device and pinned buffers of the per-thread contexts, the device follower.  Host side only.
#pragma once
#include <string>

#include "../../include/rmu.h"
#include "rmu_common.h"

// ---- error path: the calling thread's message behind rmu_last_error() (defined in rmu_api.hip) ----
extern "C" void rmu_set_error_(const char* msg);
inline int rmu_fail(int code, const std::string& msg) { rmu_set_error_(msg.c_str()); return code; }
#define RMU_HIP_TRY(expr)                                                                                           \
    do {                                                                                                            \
        hipError_t e_ = (expr);                                                                                     \
        if (e_ != hipSuccess)                                                                                       \
            return rmu_fail(e_ == hipErrorOutOfMemory ? RMU_E_OOM : RMU_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// true once the process has begun to tear the HIP runtime down (static destructors / atexit; rmu_api.hip): a thread-local destructor that
// runs after that point must not call into HIP any more
bool rmu_runtime_down();

// Grow-only device buffer of a per-thread context.  One owner: it frees itself, so a context's destructor holds only what has an order
// (wait for the work in flight, destroy events and streams) and the buffers go behind that body.
struct RmuDevBuf {
    void* p = nullptr;
    size_t cap = 0;
    RmuDevBuf() = default;
    RmuDevBuf(const RmuDevBuf&) = delete;
    RmuDevBuf& operator=(const RmuDevBuf&) = delete;
    ~RmuDevBuf() { if (p && !rmu_runtime_down()) (void)rmu_free(p); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)rmu_free(p);
        p = nullptr; cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        const hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
};

// Grow-only pinned buffer the host side of a call goes through; never smaller than `floor` bytes.  A failed allocation leaves nothing in
// the thread's last HIP error.
struct RmuPinBuf {
    char* p = nullptr;
    size_t cap = 0;
    const size_t floor;
    explicit RmuPinBuf(size_t floor_bytes) : floor(floor_bytes) {}
    RmuPinBuf(const RmuPinBuf&) = delete;
    RmuPinBuf& operator=(const RmuPinBuf&) = delete;
    ~RmuPinBuf() {
        if (!p || rmu_runtime_down()) return;
        RMU_ENTRY();
        (void)hipHostFree(p);
    }
    int ensure(size_t bytes) {
        if (bytes <= cap) return RMU_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        const size_t want = bytes < floor ? floor : bytes * 2;
        if (hipHostMalloc((void**)&p, want) != hipSuccess) { p = nullptr; (void)hipGetLastError(); return RMU_E_OOM; }
        cap = want;
        return RMU_OK;
    }
};

// the calling thread follows the device rmu_init chose; `cached` is the context's record of the device it last set
inline void rmu_follow_device(int& cached) {
    const int dev = rmu_device_ordinal();
    if (dev >= 0 && cached != dev) { (void)hipSetDevice(dev); cached = dev; }
}
