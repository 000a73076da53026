// cosine_common.h -- what the fp64 cosine units share (semantic.hip: adjacent rows; provenance.hip: member rows against one or two anchors):
// the lane's fragment of a row, the fixed-order fp64 sums, the calling thread's workspace and the error path (gfx950 only).
//
// The order of every sum is fixed by the element index alone: element e belongs to lane (e >> 2) & 63; a lane adds its elements in ascending
// order, starting from +0.0 (fma(a, b, acc) rounds once, like acc + exact product: an fp64 product of two fp32 values is exact); the 64 lane
// sums are folded by an xor butterfly over 32, 16, 8, 4, 2, 1 (every lane ends with the same bits).  A lane holds the elements
// 4 * (lane + 64 j) .. + 3, j < NJ, of a row as NJ float4 registers (NJ * 256 >= dim; elements past dim are +0.0 and add nothing), so a sum has
// the same bits in every instantiation that is wide enough and on either load path.
// Everything here has internal linkage: each unit has its own thread-local workspace.
#pragma once
#include <cstring>
#include <string>

#include "../../include/rmu.h"
#include "rmu_common.h"

extern "C" void rmu_set_error_(const char* msg);

namespace {

int cos_fail(int code, const std::string& m) { rmu_set_error_(m.c_str()); return code; }
#define COS_TRY(expr)                                                                                               \
    do {                                                                                                            \
        hipError_t e_ = (expr);                                                                                     \
        if (e_ != hipSuccess)                                                                                       \
            return cos_fail(e_ == hipErrorOutOfMemory ? RMU_E_OOM : RMU_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// the lane's NJ groups of four elements of one row; elements at or past dim are +0.0.  VEC: 16-byte loads (base 16-byte aligned, stride a
// multiple of 4 floats) for every group of four that lies inside the row; the last, partial group and the whole row otherwise take 4-byte loads
template <int NJ, bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ row, int dim, int lane, f32x4 (&f)[NJ]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = 4 * (lane + 64 * j);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (VEC && e + 4 <= dim) {
            v = *reinterpret_cast<const f32x4*>(row + e);
        } else {
            if (e < dim) v.x = row[e];
            if (e + 1 < dim) v.y = row[e + 1];
            if (e + 2 < dim) v.z = row[e + 2];
            if (e + 3 < dim) v.w = row[e + 3];
        }
        f[j] = v;
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int NJ>
__device__ __forceinline__ double lane_norm2(const f32x4 (&f)[NJ]) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double v = (double)f[j][c];
            acc = __builtin_fma(v, v, acc);
        }
    return acc;
}

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
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
bool g_cos_down = false;       // static destructors have begun: thread-local destructors must leave HIP alone
struct CosDownGuard { ~CosDownGuard() { g_cos_down = true; } } g_cos_down_guard;
// the calling thread's workspace of one unit: the uploaded rows, the results, a small table, and the pinned buffer the host side of a call
// goes through.  Only a call that drains its stream uses it, so nothing of it is ever in flight between two calls
struct CosCtx {
    DevBuf in, out, tab;
    char* pin = nullptr;
    size_t pin_cap = 0;
    int ensure_pin(size_t bytes) {
        if (bytes <= pin_cap) return RMU_OK;
        if (pin) (void)hipHostFree(pin);
        pin = nullptr; pin_cap = 0;
        const size_t cap = bytes < 8192 ? 8192 : bytes * 2;
        if (hipHostMalloc((void**)&pin, cap) != hipSuccess) { pin = nullptr; (void)hipGetLastError(); return RMU_E_OOM; }
        pin_cap = cap;
        return RMU_OK;
    }
    ~CosCtx() {
        if (g_cos_down) return;
        RMU_ENTRY();
        for (DevBuf* b : {&in, &out, &tab})
            if (b->p) (void)rmu_free(b->p);
        if (pin) (void)hipHostFree(pin);
    }
};

}  // namespace
